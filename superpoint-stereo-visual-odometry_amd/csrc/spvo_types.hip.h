// spvo_types.hip.h -- the plain structs that cross translation units: kernel-argument records the context keeps between
// calls.  The kernel headers include this file and define no such type themselves, so that a translation unit that only
// needs the context (csrc/spvo_internal.hip.h) does not pull in -- and re-define -- another unit's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spvo {

// ---- K8-K10 (post.hip.h): the NMS state map is padded (NMS_PAD rows/columns of ST_NONE on every side, row pitch a multiple
// of 4) so that a candidate's whole window is read with aligned 32-bit loads and no clipping.
constexpr int NMS_PAD = 8;           // >= largest supported dist_thresh
constexpr int NMS_MAX_LAUNCH = 16;   // round launches per host batch
constexpr int NMS_COUNTER_INTS = 8 + NMS_MAX_LAUNCH;

__host__ __device__ inline int nms_state_pitch(int W) { return ((W + 2 * NMS_PAD + 3) / 4) * 4; }

struct NmsBuffers {   // per image
  uint8_t *state;     // [(H + 2*NMS_PAD)][pitch]
  int *cand;          // [H*W] row-major pixel index of each candidate
  int *counters;      // [0] n_cand, [1] n_survivors, [2] n_out, [3] overflow, [8 + l] undecided after launch l
  unsigned long long *surv_key;  // [surv_cap]
  int *rank;          // [surv_cap], zero between uses
  int *out_xy;        // [max_kp][2]
};
struct NmsPair { NmsBuffers b[2]; };   // blockIdx.y / blockIdx.z selects the image

// the state map's values, K9's rank keys and LDS tile: the classic front end's kernels (orb.hip.h, classic_detect.hip.h) use them too
enum : uint8_t { ST_NONE = 0, ST_UNDECIDED = 1, ST_KEPT = 2, ST_SUPPRESSED = 4 };   // one bit each: word-wide tests
__device__ __forceinline__ unsigned long long rank_key(float conf, int x, int y, int H) {
  return ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(conf)) << 32) | (unsigned)(x * H + y);
}
constexpr int RANK_TILE = 1024;

// FAST-9/16 on the Bresenham circle of radius 3 around *p (row pitch w, p at least 3 pixels inside): the smallest |difference| on the best arc
// of nine contiguous circle pixels that are all brighter than the centre + t or all darker than the centre - t -- the largest threshold at
// which the pixel is still a corner, plus one -- or 0 if there is no such arc.  orb_fast_kernel's score (ORB, FAST) and, at t = 0 and less
// one, the BRISK detector's AGAST 9-16 score (brisk_detect.hip.h).
__device__ __forceinline__ int fast916_arc_score(const uint8_t *p, int w, int t) {
  int best = 0;
  const int c = *p;
  const int off[16] = {-3 * w, -3 * w + 1, -2 * w + 2, -w + 3, 3, w + 3, 2 * w + 2, 3 * w + 1, 3 * w, 3 * w - 1, 2 * w - 2, w - 3, -3, -w - 3, -2 * w - 2, -3 * w - 1};
  int d[25];
#pragma unroll
  for (int i = 0; i < 16; ++i) d[i] = (int)p[off[i]] - c;
  const int nb = (d[0] > t) + (d[4] > t) + (d[8] > t) + (d[12] > t), nd = (d[0] < -t) + (d[4] < -t) + (d[8] < -t) + (d[12] < -t);
  if (nb >= 2 || nd >= 2) {
#pragma unroll
    for (int i = 16; i < 25; ++i) d[i] = d[i - 16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      int mn = 255, mx = -255;
#pragma unroll
      for (int k = 0; k < 9; ++k) { mn = min(mn, d[s + k]); mx = max(mx, d[s + k]); }
      if (mn > t) best = max(best, mn);
      if (-mx > t) best = max(best, -mx);
    }
  }
  return best;
}

// ---- K15 (odometry.hip.h)
struct RansacWork {      // device scratch
  int *counts;           // [iterations]  (-1 = invalid hypothesis)
  double *poses;         // [iterations][7]  q(xyzw), t
  double *result;        // [8]: rvec(3), tvec(3), ok, n_inliers
  int *inliers;          // [n]
};

// ---- K16 (odometry.hip.h)
struct ObsDev {   // mirrors spvo_obs (include/spvo.h)
  float X[3];
  float uv[2];
  int32_t cam;
  int32_t inverse;
};

struct RefineOut {   // device, doubles: q(4) t(3) iterations converged usable initial_cost final_cost
  double v[12];
};

// ---- ORB (orb.hip.h)
struct OrbKeypoint { float x, y, angle, response; int32_t octave; };   // mirrors spvo_orb_keypoint (include/spvo.h)

// ---- SIFT (sift.hip.h): where the levels of an image's pyramid lie -- Gaussian layer i of octave o at pyr + g_off[o] + i * h[o] * w[o],
// difference-of-Gaussians layer i alike from d_off[o]
constexpr int SIFT_MAX_OCT = 16;
struct SiftPyr {
  float *pyr;
  long long g_off[SIFT_MAX_OCT], d_off[SIFT_MAX_OCT];
  int h[SIFT_MAX_OCT], w[SIFT_MAX_OCT];
  int n_oct;
};
// the ordering stage on the device (sift.hip.h): a raw row's sort key, and where a final row came from
struct SiftKey { float x, y, size, angle, response; int32_t octave; };   // mirrors spvo_sift_keypoint (include/spvo.h)
struct SiftSrc { int4 pos; float4 off; float angle; int pad[3]; };        // the candidate {octave, layer, row, column}, {xi, xr, xc, contrast}, the peak's angle

// ---- BRISK detector (brisk_detect.hip.h): the six layers of the scale space (layer 0 is the resident image of spvo_ctx::cls), the tap runs
// of cv::resize(INTER_AREA)'s general path, a down-sampling job and the keypoint record
constexpr int BRISK_DET_LAYERS = 6, BRISK_DET_TAPS = 6;
struct BriskDetLayer { uint8_t *im, *score; int h, w; float scale, offset; };
struct BriskDetLayers { BriskDetLayer l[BRISK_DET_LAYERS]; uint8_t *score58; };   // score58: the AGAST 5-8 score of layer 0
struct BriskAreaTap { int start, n; float a[BRISK_DET_TAPS]; };                    // sources start .. start + n - 1 with weights a[0 .. n - 1]
struct BriskResizeJob { const uint8_t *src; uint8_t *dst; int sh, sw, dh, dw; const BriskAreaTap *xtab, *ytab; };   // tabs = NULL: the exact half
struct BriskResizeJobs { BriskResizeJob j[2]; };
struct BriskDetKeypoint { float x, y, size, angle, response; int32_t octave; };   // mirrors spvo_brisk_keypoint (include/spvo.h)

// ---- AKAZE detector (akaze.hip.h): a level of the nonlinear scale space with its resident planes (the four spvo_akaze_debug_level serves,
// and the scaled first derivatives Lx, Ly of rule 9, which the descriptor of akaze_mldb.hip.h samples), the symmetric half of a Gaussian
// kernel, a candidate as the extrema stage leaves it for the host's suppression (its first seven fields mirror spvo_akaze_keypoint), and
// that record itself as the describe kernel reads it
constexpr int AKAZE_MAX_LEVELS = 16, AKAZE_MAX_OCTAVES = 4, AKAZE_BLUR_R = 4, AKAZE_NBINS = 300;
struct AkazeLevel { float *Lt, *Lsmooth, *Lflow, *Ldet, *Lx, *Ly; int h, w, octave, sigma_size, border; float esigma; };
struct AkazeLevels { AkazeLevel l[AKAZE_MAX_LEVELS]; int n; };
struct AkazeTaps { float g[AKAZE_BLUR_R + 1]; int r; };   // g[0] the centre, g[j] the taps at +- j, j <= r
struct AkazeCand { float x, y, size, angle, response; int32_t octave, class_id, row, col, ok; };
struct AkazeKp { float x, y, size, angle, response; int32_t octave, class_id; };
// the integers of a call (one cleared allocation): candidates, overflow flag, bits of the gradient maximum, the contrast factor per octave
// (float bits), the histogram
constexpr int AKAZE_STAT_NCAND = 0, AKAZE_STAT_OVERFLOW = 1, AKAZE_STAT_MAX = 2, AKAZE_STAT_K = 4, AKAZE_STAT_HIST = 8, AKAZE_STAT_INTS = AKAZE_STAT_HIST + AKAZE_NBINS;

// ---- the link from a detector's record list to the octave-aware ORB extractor (orb_link.hip.h): where the list lies -- records of
// `stride` bytes with x, y (float) and the octave (int32) at byte offsets, an optional keep flag per record, the list's length on the
// device and what the buffer holds at most
struct OrbLinkSrc { const char *rec; int stride, off_x, off_y, off_octave; const int *keep; const int *n_ptr; int n_cap; };

// ---- the link from a detector's record list to the SIFT extractor (sift.hip.h: spvo_brisk_sift_pair, spvo_akaze_sift_pair,
// spvo_sift_link_debug): the same description of where the list lies, with every field the extractor reads (x, y, size, angle, response:
// float; octave: int32) at its byte offset -- `stride` is a multiple of 4, the whole record travels to the host's mirror -- and where the
// detector's overflow flag is: det_counters[3] (BRISK; ORB through orb_records_kernel's block), or stat (AKAZE_STAT_*) against cand_cap (AKAZE), or neither
struct SiftLinkSrc {
  const char *rec;
  int stride, off_x, off_y, off_size, off_angle, off_response, off_octave;
  const int *keep, *n_ptr;
  int n_cap;
  const int *det_counters, *stat;
  int cand_cap;
};

}  // namespace spvo
