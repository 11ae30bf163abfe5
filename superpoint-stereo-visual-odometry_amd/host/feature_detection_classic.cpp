// feature_detection_classic.cpp -- ClassicFeatureFrontEnd: the bookkeeping the reference does in
//   src/odml_visual_odometry/src/feature_detection_classic.cpp  ("classic.cpp")
// beside feature_detection.cpp (base.cpp and nn.cpp); the same conventions.
#include "feature_detection.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

// ------------------------------------------------------------------------- classic front end (classic.cpp)
static bool g_classic_resident = false;
static int g_classic_resident_capacity = 8192;
static bool g_classic_brisk_pair_resident = false;
static bool g_classic_akaze_descriptor = false;
static bool g_classic_akaze_pair_resident = false;
static bool g_classic_sift_describe_resident = false;
static bool g_classic_orb_octaves = false;
static bool g_classic_octave_pairs_resident = false;
static bool g_classic_sift_octave_pairs_resident = false;
static bool g_classic_orb_brisk = false;
static bool g_classic_orb_pairs_resident = false;
static bool g_classic_sift_brisk = false;
static bool g_classic_sift_brisk_resident = false;
void ClassicFeatureFrontEnd::setDeviceResident(bool on) { g_classic_resident = on; }
void ClassicFeatureFrontEnd::setBriskPairResident(bool on) { g_classic_brisk_pair_resident = on; }
void ClassicFeatureFrontEnd::setAkazeDescriptor(bool on) { g_classic_akaze_descriptor = on; }
void ClassicFeatureFrontEnd::setAkazePairResident(bool on) { g_classic_akaze_pair_resident = on; }
void ClassicFeatureFrontEnd::setSiftDescribeResident(bool on) { g_classic_sift_describe_resident = on; }
void ClassicFeatureFrontEnd::setOrbExtractorOctaves(bool on) { g_classic_orb_octaves = on; }
void ClassicFeatureFrontEnd::setOctavePairsResident(bool on) { g_classic_octave_pairs_resident = on; }
void ClassicFeatureFrontEnd::setSiftOctavePairsResident(bool on) { g_classic_sift_octave_pairs_resident = on; }
void ClassicFeatureFrontEnd::setOrbBriskExtractor(bool on) { g_classic_orb_brisk = on; }
void ClassicFeatureFrontEnd::setOrbPairsResident(bool on) { g_classic_orb_pairs_resident = on; }
void ClassicFeatureFrontEnd::setSiftBriskExtractor(bool on) { g_classic_sift_brisk = on; }
void ClassicFeatureFrontEnd::setSiftBriskResident(bool on) { g_classic_sift_brisk_resident = on; }
void ClassicFeatureFrontEnd::setResidentCapacity(int rows) { g_classic_resident_capacity = rows; }

#ifdef SPVO_USE_OPENCV
bool ClassicFeatureFrontEnd::available() { return true; }
bool ClassicFeatureFrontEnd::pairRuns() const { return true; }
bool ClassicFeatureFrontEnd::addStereoImagePairResident(cv::Mat &, cv::Mat &) { return false; }   // (the OpenCV detectors work on the host)

void ClassicFeatureFrontEnd::initDetector() {   // parameters: classic.cpp:7-56
  if (detector_type_ == DetectorType::ORB) detector_ = cv::ORB::create(2000, 1.2f, 8, 31, 0, 2, cv::ORB::FAST_SCORE, 31, 20);
  else if (detector_type_ == DetectorType::BRISK) detector_ = cv::BRISK::create();
  else if (detector_type_ == DetectorType::AKAZE) detector_ = cv::AKAZE::create();
  else if (detector_type_ == DetectorType::SIFT) detector_ = cv::SIFT::create();
  else if (detector_type_ == DetectorType::FAST) detector_ = cv::FastFeatureDetector::create(10, true);
  else if (detector_type_ == DetectorType::ShiTomasi) detector_ = cv::GFTTDetector::create(1000, 0.03, 7.5, 5, false, 0.04);
  else logError("[initDetector] Detector is not implemented");
}

void ClassicFeatureFrontEnd::initDescriptor() {   // classic.cpp:58-79
  if (descriptor_type_ == DescriptorType::ORB) extractor_ = cv::ORB::create();
  else if (descriptor_type_ == DescriptorType::BRISK) extractor_ = cv::BRISK::create(30, 3, 1.0f);
  else if (descriptor_type_ == DescriptorType::AKAZE) extractor_ = cv::AKAZE::create();
  else if (descriptor_type_ == DescriptorType::SIFT) extractor_ = cv::SIFT::create();
  else logError("[initDescriptor] Decscriptor is not implemented");
}

std::vector<cv::KeyPoint> ClassicFeatureFrontEnd::detectKeypoints(const cv::Mat &img) {
  std::vector<cv::KeyPoint> keypoints;
  if (detector_) detector_->detect(img, keypoints);
  return keypoints;
}

cv::Mat ClassicFeatureFrontEnd::describeKeypoints(std::vector<cv::KeyPoint> &keypoints, const cv::Mat &img) {
  cv::Mat descriptors;
  if (extractor_) extractor_->compute(img, keypoints, descriptors);
  return descriptors;
}

void ClassicFeatureFrontEnd::addStereoImagePair(cv::Mat &img_l, cv::Mat &img_r, const cv::Mat &projection_matrix_l, const cv::Mat &projection_matrix_r) {
  if (img_l.rows != img_r.rows || img_l.cols != img_r.cols) {
    logError("input images shape doesn't match!");
    return;
  }
  projection_matrix_l_ = projection_matrix_l.clone();
  projection_matrix_r_ = projection_matrix_r.clone();
  if (input_height_ > 0 && input_width_ > 0) {   // 0 = native resolution (launch/visual_odometry_classic.launch)
    preprocessImageImpl(img_l, projection_matrix_l_);
    preprocessImageImpl(img_r, projection_matrix_r_);
  }
  cv::Mat *imgs[2] = {&img_l, &img_r};
  for (cv::Mat *im : imgs) {
    images_dq.push_back(*im);
    keypoints_dq.push_back(detectKeypoints(*im));
    descriptors_dq.push_back(describeKeypoints(keypoints_dq.back(), *im));
  }
  if (verbose_) logInfo(std::to_string(keypoints_dq.end()[-2].size()) + ", " + std::to_string(keypoints_dq.end()[-1].size()) + " keypoints for img_l and img_r");
  while (images_dq.size() > NUM_IMAGE_POSITIONS) {
    images_dq.pop_front();
    keypoints_dq.pop_front();
    descriptors_dq.pop_front();
  }
}
#else
// Without OpenCV the pairs of kClassicPairs run, on the GPU, and every other combination is refused.  What the table cannot say: ORB + ORB and
// SIFT + SIFT describe in the detector's pass, so detectKeypoints keeps the rows for the describeKeypoints call that follows on the same image;
// every other detector leaves the image (AKAZE: its scale space) on the device for the extractor -- except ORB, which keeps a pyramid of its
// own: the per-image path of ORB + SIFT and ORB + BRISK uploads the image a second time (their resident routes, spvo_orb_sift_pair and
// spvo_orb_brisk_pair, run the detector on the shared resident image) -- and SIFT, which keeps an image of its own as well: the per-image
// path of SIFT + BRISK uploads twice and discards the detector's 128-float rows (spvo_sift_brisk_pair builds the pyramid from the shared
// resident image and computes no SIFT row).  The AKAZE extractor needs the level in
// class_id, which only AKAZE keypoints carry -- OpenCV's own assertion refuses the others too.
bool ClassicFeatureFrontEnd::available() { return true; }

enum class Detect { Orb, Gftt, Fast, Sift, Brisk, Akaze };       // detectKeypoints: spvo_<this>_detect
enum class Describe { WithDetector, Orb, Brisk, Akaze, Sift };   // describeKeypoints: the rows detectKeypoints kept, or spvo_<this>_describe on the given keypoints
enum class Route { None, Classic, SiftPair, BriskPair, AkazePair, ClassicSift, BriskOrbPair, AkazeOrbPair, AkazeBriskPair, BriskSiftPair, AkazeSiftPair, OrbBriskPair, OrbSiftPair, SiftBriskPair };   // setDeviceResident: the per-image path, spvo_classic_detect (kind), spvo_sift_detect_pair, spvo_brisk_detect_pair, spvo_akaze_detect_pair, spvo_classic_sift_pair (kind), spvo_brisk_orb_pair, spvo_akaze_orb_pair, spvo_akaze_brisk_pair, spvo_brisk_sift_pair, spvo_akaze_sift_pair, spvo_orb_brisk_pair, spvo_orb_sift_pair, spvo_sift_brisk_pair
enum class OptIn { None, AkazeDescriptor, OrbOctaves, BriskPairResident, AkazePairResident, SiftDescribeResident, OctavePairsResident, SiftOctavePairsResident, OrbBrisk, OrbPairsResident, SiftBrisk, SiftBriskResident };   // to run at all: setAkazeDescriptor, setOrbExtractorOctaves, setOrbBriskExtractor, setSiftBriskExtractor; to stay resident: setBriskPairResident, setAkazePairResident, setSiftDescribeResident, setOctavePairsResident, setSiftOctavePairsResident, setOrbPairsResident, setSiftBriskResident

struct ClassicPair {
  DetectorType detector;
  DescriptorType descriptor;
  Detect detect;
  float keypoint_size;   // of a corner: KeyPoint::convert(corners, keypoints, blockSize = 5) / KeyPoint(x, y, 7.f, -1, score); 0: the detector reports it
  Describe describe;
  int cols, type;        // a descriptor row; CV_8UC1 rows are matched with NORM_HAMMING, CV_32FC1 rows with NORM_L2
  Route route;
  int kind;              // Route::Classic, Route::ClassicSift: the spvo_classic_kind
  OptIn opt_in;          // what the pair needs to run at all ...
  OptIn resident_opt_in; // ... and what its route needs beside setDeviceResident
  size_t rowBytes() const { return (size_t)cols * (type == CV_32FC1 ? sizeof(float) : 1); }
};
static const ClassicPair kClassicPairs[] = {
    {DetectorType::ORB, DescriptorType::ORB, Detect::Orb, 0.f, Describe::WithDetector, 32, CV_8UC1, Route::Classic, SPVO_CLASSIC_ORB, OptIn::None, OptIn::None},
    {DetectorType::ShiTomasi, DescriptorType::ORB, Detect::Gftt, 5.f, Describe::Orb, 32, CV_8UC1, Route::Classic, SPVO_CLASSIC_GFTT_ORB, OptIn::None, OptIn::None},
    {DetectorType::FAST, DescriptorType::ORB, Detect::Fast, 7.f, Describe::Orb, 32, CV_8UC1, Route::Classic, SPVO_CLASSIC_FAST_ORB, OptIn::None, OptIn::None},
    {DetectorType::ShiTomasi, DescriptorType::BRISK, Detect::Gftt, 5.f, Describe::Brisk, 64, CV_8UC1, Route::Classic, SPVO_CLASSIC_GFTT_BRISK, OptIn::None, OptIn::None},
    {DetectorType::FAST, DescriptorType::BRISK, Detect::Fast, 7.f, Describe::Brisk, 64, CV_8UC1, Route::Classic, SPVO_CLASSIC_FAST_BRISK, OptIn::None, OptIn::None},
    {DetectorType::BRISK, DescriptorType::BRISK, Detect::Brisk, 0.f, Describe::Brisk, 64, CV_8UC1, Route::BriskPair, 0, OptIn::None, OptIn::BriskPairResident},
    {DetectorType::AKAZE, DescriptorType::BRISK, Detect::Akaze, 0.f, Describe::Brisk, 64, CV_8UC1, Route::AkazeBriskPair, 0, OptIn::None, OptIn::OctavePairsResident},
    {DetectorType::AKAZE, DescriptorType::AKAZE, Detect::Akaze, 0.f, Describe::Akaze, SPVO_AKAZE_DESC_BYTES, CV_8UC1, Route::AkazePair, 0, OptIn::AkazeDescriptor, OptIn::AkazePairResident},
    {DetectorType::SIFT, DescriptorType::SIFT, Detect::Sift, 0.f, Describe::WithDetector, 128, CV_32FC1, Route::SiftPair, 0, OptIn::None, OptIn::None},
    {DetectorType::ShiTomasi, DescriptorType::SIFT, Detect::Gftt, 5.f, Describe::Sift, 128, CV_32FC1, Route::ClassicSift, SPVO_CLASSIC_GFTT_SIFT, OptIn::None, OptIn::SiftDescribeResident},
    {DetectorType::FAST, DescriptorType::SIFT, Detect::Fast, 7.f, Describe::Sift, 128, CV_32FC1, Route::ClassicSift, SPVO_CLASSIC_FAST_SIFT, OptIn::None, OptIn::SiftDescribeResident},
    // (spvo_orb_sift_pair runs the ORB detector on the shared resident image; the per-image path keeps spvo_orb_detect's own pyramid and image)
    {DetectorType::ORB, DescriptorType::SIFT, Detect::Orb, 0.f, Describe::Sift, 128, CV_32FC1, Route::OrbSiftPair, 0, OptIn::None, OptIn::OrbPairsResident},
    {DetectorType::BRISK, DescriptorType::SIFT, Detect::Brisk, 0.f, Describe::Sift, 128, CV_32FC1, Route::BriskSiftPair, 0, OptIn::None, OptIn::SiftOctavePairsResident},
    {DetectorType::AKAZE, DescriptorType::SIFT, Detect::Akaze, 0.f, Describe::Sift, 128, CV_32FC1, Route::AkazeSiftPair, 0, OptIn::None, OptIn::SiftOctavePairsResident},
    // the ORB extractor on keypoints that carry an octave (spvo_orb_describe_octaves): only with setOrbExtractorOctaves, and listed only then
    {DetectorType::BRISK, DescriptorType::ORB, Detect::Brisk, 0.f, Describe::Orb, 32, CV_8UC1, Route::BriskOrbPair, 0, OptIn::OrbOctaves, OptIn::OctavePairsResident},
    {DetectorType::AKAZE, DescriptorType::ORB, Detect::Akaze, 0.f, Describe::Orb, 32, CV_8UC1, Route::AkazeOrbPair, 0, OptIn::OrbOctaves, OptIn::OctavePairsResident},
    // the BRISK extractor on ORB keypoints (size 31 x 1.2^octave): only with setOrbBriskExtractor, and listed only then
    {DetectorType::ORB, DescriptorType::BRISK, Detect::Orb, 0.f, Describe::Brisk, 64, CV_8UC1, Route::OrbBriskPair, 0, OptIn::OrbBrisk, OptIn::OrbPairsResident},
    // the BRISK extractor on SIFT keypoints (their own size; one keypoint per orientation peak, as OpenCV's detector emits them): only with
    // setSiftBriskExtractor, and listed only then
    {DetectorType::SIFT, DescriptorType::BRISK, Detect::Sift, 0.f, Describe::Brisk, 64, CV_8UC1, Route::SiftBriskPair, 0, OptIn::SiftBrisk, OptIn::SiftBriskResident},
};
// the run-at-all switches of a front end, as its constructor read them
struct ClassicOptIns { bool akaze_descriptor, orb_octaves, orb_brisk, sift_brisk; };
static bool opted_in(const ClassicPair &p, const ClassicOptIns &o) {
  return (p.opt_in != OptIn::AkazeDescriptor || o.akaze_descriptor) && (p.opt_in != OptIn::OrbOctaves || o.orb_octaves) && (p.opt_in != OptIn::OrbBrisk || o.orb_brisk) &&
         (p.opt_in != OptIn::SiftBrisk || o.sift_brisk);
}

// the row of a pair that runs, or nullptr
static const ClassicPair *find_pair(DetectorType d, DescriptorType e, const ClassicOptIns &o) {
  for (const ClassicPair &p : kClassicPairs)
    if (p.detector == d && p.descriptor == e && opted_in(p, o)) return &p;
  return nullptr;
}
ClassicOptIns ClassicFeatureFrontEnd::optIns() const { return ClassicOptIns{akaze_descriptor_, orb_octaves_, orb_brisk_, sift_brisk_}; }
const ClassicPair *ClassicFeatureFrontEnd::pair() const { return find_pair(detector_type_, descriptor_type_, optIns()); }
bool ClassicFeatureFrontEnd::pairRuns() const { return pair() != nullptr; }

template <class Names, class T> static std::string name_of(const Names &names, T type) {
  for (const auto &kv : names)
    if (kv.second == type) return kv.first;
  return "?";
}
// what a pair that does not run is told: the table's rows (those behind setOrbExtractorOctaves / setOrbBriskExtractor / setSiftBriskExtractor only while that switch is on)
static std::string refusal(const ClassicOptIns &o) {
  std::string s = "this detector / descriptor pair is an OpenCV features2d call (classic.cpp:7-79) -- built without SPVO_USE_OPENCV, only these pairs run: ";
  for (const ClassicPair &p : kClassicPairs) {
    if ((p.opt_in == OptIn::OrbOctaves && !o.orb_octaves) || (p.opt_in == OptIn::OrbBrisk && !o.orb_brisk) || (p.opt_in == OptIn::SiftBrisk && !o.sift_brisk)) continue;
    s += std::string(&p == kClassicPairs ? "" : ", ") + name_of(detector_name_to_type, p.detector) + " + " + name_of(descriptor_name_to_type, p.descriptor) +
         (p.opt_in == OptIn::AkazeDescriptor ? " (with setAkazeDescriptor)" : "");
  }
  return s;
}
// Of a pair that does not run, the detector is at fault unless it runs with the ORB extractor, and the descriptor unless it runs on ORB
// keypoints (ORB + ORB is the reference's baseline, launch/visual_odometry_classic.launch)
void ClassicFeatureFrontEnd::initDetector() {
  if (!pair() && !find_pair(detector_type_, DescriptorType::ORB, optIns())) logError("[initDetector] " + refusal(optIns()));
}
void ClassicFeatureFrontEnd::initDescriptor() {
  if (!pair() && !find_pair(DetectorType::ORB, descriptor_type_, optIns())) logError("[initDescriptor] " + refusal(optIns()));
}

// ---- records -> cv::KeyPoint: one conversion per record type, for the per-image path and the resident one alike
static float orb_degrees(float radians) {   // spvo_orb_* report radians; cv::KeyPoint::angle is in degrees, 0 .. 360
  const float a = radians * 57.29577951308232f;
  return a < 0 ? a + 360.f : a;
}
// (extracted: the record is a pair call's and carries its extractor's angle, not the detector's)
static cv::KeyPoint to_keypoint(const spvo_orb_keypoint &r, const ClassicPair &p, bool /*extracted*/) {
  static const std::array<float, 8> level_scale = [] {   // cv::ORB::create(2000, 1.2f, 8, ..)
    std::array<float, 8> s{};
    s[0] = 1.f;
    for (int l = 1; l < 8; ++l) s[l] = s[l - 1] * 1.2f;
    return s;
  }();
  cv::KeyPoint k(cv::Point2f(r.x, r.y), p.detect == Detect::Orb ? 31.f * level_scale[r.octave & 7] : p.keypoint_size);
  // (the BRISK kinds of spvo_classic_detect report the extractor's degrees, taken as they are; ORB + BRISK's record is spvo_orb_detect's: radians)
  k.angle = p.describe == Describe::Brisk && p.detect != Detect::Orb ? r.angle : orb_degrees(r.angle);
  k.response = r.response;
  k.octave = r.octave;
  return k;
}
static cv::KeyPoint to_keypoint(float x, float y, float response, const ClassicPair &p) {   // spvo_gftt_detect / spvo_fast_detect: xy + response
  cv::KeyPoint k(cv::Point2f(x, y), p.keypoint_size);
  k.angle = -1.f;
  k.response = response;
  k.octave = 0;
  return k;
}
static cv::KeyPoint to_keypoint(const spvo_sift_keypoint &r, const ClassicPair &p, bool extracted) {   // SIFT (SIFT + BRISK: spvo_sift_detect's record per image -- describeKeypoints replaces the angle -- and spvo_sift_brisk_pair's, which carries the extractor's degrees; octave stays SIFT's packed field), BRISK's records of the same layout, and spvo_classic_sift_pair's
                                                                                       // (size 5 / 7, angle -1, octave 0: what to_keypoint(x, y, response, p) builds)
  cv::KeyPoint k(cv::Point2f(r.x, r.y), r.size);
  // a BRISK keypoint keeps the angle its detector reports, -1; the record of spvo_brisk_detect_pair carries the extractor's, which stays with the slot.
  // The ORB extractor's angle replaces it (spvo_brisk_orb_pair's record: radians), as describeKeypoints does
  k.angle = extracted && p.describe == Describe::Orb ? orb_degrees(r.angle) : p.detect == Detect::Brisk ? -1.f : r.angle;
  k.response = r.response;
  k.octave = r.octave;   // BRISK: the layer, 0 .. 5
  return k;
}
static cv::KeyPoint to_keypoint(const spvo_akaze_keypoint &r, const ClassicPair &p, bool extracted) {
  cv::KeyPoint k(cv::Point2f(r.x, r.y), r.size);
  k.angle = extracted && p.describe == Describe::Orb ? orb_degrees(r.angle) : r.angle;   // the detector's 0 (the orientation belongs to the descriptor stage), a pair call's degrees, or spvo_akaze_orb_pair's radians
  k.response = r.response;
  k.octave = r.octave;
  k.class_id = r.class_id;   // the level, 0 .. 15
  return k;
}
template <class Record> static std::vector<cv::KeyPoint> to_keypoints(const Record *r, int n, const ClassicPair &p, bool extracted = false) {
  std::vector<cv::KeyPoint> keypoints;
  keypoints.reserve(n);
  for (int i = 0; i < n; ++i) keypoints.push_back(to_keypoint(r[i], p, extracted));
  return keypoints;
}
// the first n of a buffer of the pair's descriptor rows, as a matrix of their own
static cv::Mat copy_rows(const void *rows, int n, const ClassicPair &p) {
  cv::Mat d(n, p.cols, p.type);
  if (n) std::memcpy(d.data, rows, (size_t)n * p.rowBytes());
  return d;
}

static bool image_ok(const cv::Mat &img) { return img.depth() == CV_8U && img.rows > 0; }

// SIFT, BRISK and AKAZE report n > cap when the buffers held fewer than there are: once more with room for all.  call(cap) sizes them and detects into n
template <class Call> static int grow_and_retry(int cap, const int &n, Call call) {
  for (;;) {
    const int rc = call(cap);
    if (rc != SPVO_OK || n <= cap) return rc;
    cap = n;
  }
}

std::vector<cv::KeyPoint> ClassicFeatureFrontEnd::detectKeypoints(const cv::Mat &img) {
  std::vector<cv::KeyPoint> keypoints;
  orb_desc_ = cv::Mat();
  detected_data_ = nullptr;
  const ClassicPair *p = pair();
  if (!p) {
    logError("ClassicFeatureFrontEnd: " + refusal(optIns()));
    return keypoints;
  }
  if (!ensureContext()) return keypoints;
  if (!image_ok(img)) {
    logError("detectKeypoints: 8-bit single-channel image expected");
    return keypoints;
  }
  const uint8_t *px = img.ptr<uint8_t>(0);
  const size_t step = (size_t)img.step;
  const char *call = "";
  int rc = SPVO_OK, n = 0;
  switch (p->detect) {
  case Detect::Orb: {
    constexpr int NFEATURES = 2000;   // classic.cpp:13
    std::vector<spvo_orb_keypoint> kp(NFEATURES);
    cv::Mat desc(NFEATURES, 32, CV_8UC1);   // ORB's own rows, whatever the pair's extractor is
    call = "spvo_orb_detect";
    rc = spvo_orb_detect(ctx_, px, img.rows, img.cols, step, NFEATURES, kp.data(), desc.ptr<uint8_t>(0), NFEATURES, &n);
    if (rc == SPVO_OK) {
      keypoints = to_keypoints(kp.data(), n, *p);
      if (p->describe == Describe::WithDetector) orb_desc_ = copy_rows(desc.data, n, *p);   // (ORB + SIFT, ORB + BRISK: the rows are not kept)
    }
    break;
  }
  case Detect::Gftt:
  case Detect::Fast: {
    // cv::GFTTDetector::create(1000, 0.03, 7.5, 5, false, 0.04) / cv::FastFeatureDetector::create(10, true), classic.cpp:32-47
    const bool gftt = p->detect == Detect::Gftt;
    const int cap = gftt ? 1000 : (img.rows / 2 + 1) * (img.cols / 2 + 1);
    std::vector<float> xy((size_t)cap * 2), resp((size_t)cap);
    call = gftt ? "spvo_gftt_detect" : "spvo_fast_detect";
    rc = gftt ? spvo_gftt_detect(ctx_, px, img.rows, img.cols, step, 1000, 0.03, 7.5, 5, xy.data(), resp.data(), cap, &n)
              : spvo_fast_detect(ctx_, px, img.rows, img.cols, step, 10, 1, xy.data(), resp.data(), cap, &n);
    if (rc == SPVO_OK) {
      n = std::min(n, cap);
      keypoints.reserve(n);
      for (int i = 0; i < n; ++i) keypoints.push_back(to_keypoint(xy[2 * i], xy[2 * i + 1], resp[i], *p));
    }
    break;
  }
  case Detect::Sift: {   // cv::SIFT::create()
    std::vector<spvo_sift_keypoint> kp;
    cv::Mat desc;
    call = "spvo_sift_detect";
    rc = grow_and_retry(4096, n, [&](int cap) {
      kp.resize((size_t)cap);
      desc = cv::Mat(cap, 128, CV_32FC1);   // SIFT's own rows, whatever the pair's extractor is
      return spvo_sift_detect(ctx_, px, img.rows, img.cols, step, kp.data(), desc.ptr<float>(0), cap, &n);
    });
    if (rc == SPVO_OK) {
      keypoints = to_keypoints(kp.data(), n, *p);
      if (p->describe == Describe::WithDetector) orb_desc_ = copy_rows(desc.data, n, *p);   // (SIFT + BRISK: the rows are not kept)
    }
    break;
  }
  case Detect::Brisk: {   // cv::BRISK::create(): threshold 30, 3 octaves (classic.cpp:9-11)
    std::vector<spvo_brisk_keypoint> kp;
    call = "spvo_brisk_detect";
    rc = grow_and_retry(4096, n, [&](int cap) {
      kp.resize((size_t)cap);
      return spvo_brisk_detect(ctx_, px, img.rows, img.cols, step, 30, 3, kp.data(), cap, &n);
    });
    if (rc == SPVO_OK) keypoints = to_keypoints(kp.data(), n, *p);
    break;
  }
  case Detect::Akaze: {
    // cv::AKAZE::create(): threshold 0.001 (classic.cpp:26-28).  A second pass runs the whole chain again, so the first buffer is generous:
    // the 375 x 1242 sample gives 1442 keypoints
    std::vector<spvo_akaze_keypoint> kp;
    call = "spvo_akaze_detect";
    rc = grow_and_retry(16384, n, [&](int cap) {
      kp.resize((size_t)cap);
      return spvo_akaze_detect(ctx_, px, img.rows, img.cols, step, 0.001f, kp.data(), cap, &n);
    });
    if (rc == SPVO_OK) keypoints = to_keypoints(kp.data(), n, *p);
    break;
  }
  }
  if (rc != SPVO_OK) {
    logError(std::string(call) + ": " + spvo_last_error(ctx_));
    return keypoints;
  }
  // (spvo_orb_detect works on a pyramid of its own and spvo_sift_detect on an image of its own: neither leaves one where the extractors look)
  if (p->describe != Describe::WithDetector && p->detect != Detect::Orb && p->detect != Detect::Sift) { detected_data_ = img.data; detected_rows_ = img.rows; detected_cols_ = img.cols; }   // still on the device for describeKeypoints
  return keypoints;
}

cv::Mat ClassicFeatureFrontEnd::describeKeypoints(std::vector<cv::KeyPoint> &keypoints, const cv::Mat &img) {
  const ClassicPair *p = pair();
  if (!p || p->describe == Describe::WithDetector) {
    if (orb_desc_.rows != (int)keypoints.size()) {
      logError("describeKeypoints: call detectKeypoints on the same image first (ORB and SIFT detect and describe in one pass here)");
      return cv::Mat();
    }
    return orb_desc_;
  }
  if (!ensureContext()) return cv::Mat();
  if (!image_ok(img)) {
    logError("describeKeypoints: 8-bit single-channel image expected");
    return cv::Mat();
  }
  // the image detectKeypoints saw last is still on the device (AKAZE: its scale space): NULL instead of a second upload (AKAZE: build)
  const bool same_image = detected_data_ && detected_data_ == img.data && detected_rows_ == img.rows && detected_cols_ == img.cols;
  const uint8_t *px = same_image ? nullptr : img.ptr<uint8_t>(0);
  const size_t step = (size_t)img.step;
  const int n = (int)keypoints.size();
  std::vector<float> angle((size_t)n);
  cv::Mat desc(n, p->cols, p->type);
  uint8_t *rows = n ? desc.ptr<uint8_t>(0) : nullptr;
  const char *call;
  int rc;
  if (p->describe == Describe::Sift) {
    // cv::SIFT::create()->compute(img, keypoints, descriptors), classic.cpp:71-73: the keypoints go in as they are -- pt, size, angle in
    // degrees (-1 from the detectors that report none), response, octave -- every one gets a row of 128 floats, none is erased and no angle
    // is changed
    std::vector<spvo_sift_keypoint> kp((size_t)n);
    for (int i = 0; i < n; ++i) kp[i] = spvo_sift_keypoint{keypoints[i].pt.x, keypoints[i].pt.y, keypoints[i].size, keypoints[i].angle, keypoints[i].response, keypoints[i].octave};
    call = "spvo_sift_describe";
    rc = spvo_sift_describe(ctx_, px, img.rows, img.cols, step, kp.data(), n, n ? desc.ptr<float>(0) : nullptr);
    if (rc == SPVO_OK) return desc;
  } else if (p->describe == Describe::Akaze) {
    // cv::AKAZE::create()->compute(img, keypoints, descriptors), classic.cpp:69-70: every keypoint gets its main orientation (degrees) and a
    // 61-byte row; none is erased.  The level comes from class_id, as in OpenCV.
    std::vector<spvo_akaze_keypoint> kp((size_t)n);
    for (int i = 0; i < n; ++i)
      kp[i] = spvo_akaze_keypoint{keypoints[i].pt.x, keypoints[i].pt.y, keypoints[i].size, keypoints[i].angle, keypoints[i].response, keypoints[i].octave, keypoints[i].class_id};
    call = "spvo_akaze_describe";
    rc = spvo_akaze_describe(ctx_, px, img.rows, img.cols, step, kp.data(), n, angle.data(), rows);
    if (rc == SPVO_OK) {
      for (int i = 0; i < n; ++i) keypoints[i].angle = angle[i];
      return desc;
    }
  } else {
    // cv::ORB::create()->compute (classic.cpp:66-68) / cv::BRISK::create(30, 3, 1.0f)->compute (classic.cpp:56-65): keypoints too close to a
    // border are ERASED from the caller's vector (it is passed by non-const reference, classic.cpp:110-111), so keypoints_dq and descriptors_dq
    // stay aligned.  BRISK: every keypoint's own size (5: ShiTomasi, 7: FAST, 12 x its scale: BRISK, 3 x esigma: AKAZE, 31 x 1.2^octave: ORB, SIFT: 1.6 x 2^((layer + xi) / 3 + octave), the detector's own) picks its scale, and the
    // angle comes in degrees, 0 .. 360 -- except that a BRISK keypoint keeps the angle its detector reports (-1)
    // ORB on BRISK / AKAZE keypoints (the rows behind setOrbExtractorOctaves): KeyPoint::octave names the pyramid level, the survivors come
    // grouped by level as OpenCV leaves them
    const bool brisk = p->describe == Describe::Brisk, octaves = p->opt_in == OptIn::OrbOctaves;
    std::vector<float> xy((size_t)n * 2), size(brisk ? (size_t)n : 0);
    std::vector<int32_t> kept((size_t)n), octave(octaves ? (size_t)n : 0);
    for (int i = 0; i < n; ++i) {
      xy[2 * i] = keypoints[i].pt.x; xy[2 * i + 1] = keypoints[i].pt.y;
      if (brisk) size[i] = keypoints[i].size;
      if (octaves) octave[i] = keypoints[i].octave;
    }
    int m = 0;
    call = brisk ? "spvo_brisk_describe" : octaves ? "spvo_orb_describe_octaves" : "spvo_orb_describe";
    rc = brisk     ? spvo_brisk_describe(ctx_, px, img.rows, img.cols, step, xy.data(), size.data(), n, kept.data(), angle.data(), rows, nullptr, &m)
         : octaves ? spvo_orb_describe_octaves(ctx_, px, img.rows, img.cols, step, xy.data(), octave.data(), n, kept.data(), angle.data(), rows, &m)
                   : spvo_orb_describe(ctx_, px, img.rows, img.cols, step, xy.data(), n, kept.data(), angle.data(), rows, &m);
    if (rc == SPVO_OK) {
      std::vector<cv::KeyPoint> out;
      out.reserve(m);
      for (int i = 0; i < m; ++i) {
        cv::KeyPoint k = keypoints[kept[i]];
        if (!brisk) k.angle = orb_degrees(angle[i]);
        else if (p->detect != Detect::Brisk) k.angle = angle[i];
        out.push_back(k);
      }
      keypoints.swap(out);
      return copy_rows(desc.data, m, *p);
    }
  }
  logError(std::string(call) + ": " + spvo_last_error(ctx_));
  keypoints.clear();
  return cv::Mat();
}

void ClassicFeatureFrontEnd::addStereoImagePair(cv::Mat &img_l, cv::Mat &img_r, const cv::Mat &projection_matrix_l, const cv::Mat &projection_matrix_r) {
  if (img_l.rows != img_r.rows || img_l.cols != img_r.cols) {
    logError("input images shape doesn't match!");
    return;
  }
  if (!pairRuns()) {
    logError("ClassicFeatureFrontEnd: " + refusal(optIns()));
    return;
  }
  if (!ensureContext()) return;   // no device: logged, nothing pushed (nn.cpp:53-55 convention)
  projection_matrix_l_ = projection_matrix_l.clone();
  projection_matrix_r_ = projection_matrix_r.clone();
  if (input_height_ > 0 && input_width_ > 0) {   // 0 = native resolution (launch/visual_odometry_classic.launch)
    preprocessImageImpl(img_l, projection_matrix_l_);
    preprocessImageImpl(img_r, projection_matrix_r_);
  }
  if (!resident_ || !addStereoImagePairResident(img_l, img_r)) {
    cv::Mat *imgs[2] = {&img_l, &img_r};
    for (cv::Mat *im : imgs) {
      images_dq.push_back(*im);
      keypoints_dq.push_back(detectKeypoints(*im));
      descriptors_dq.push_back(describeKeypoints(keypoints_dq.back(), *im));
      if (resident_) bin_slots_dq_.push_back(-1);   // on the host only
    }
  }
  if (verbose_) logInfo(std::to_string(keypoints_dq.end()[-2].size()) + ", " + std::to_string(keypoints_dq.end()[-1].size()) + " keypoints for img_l and img_r");
  while (images_dq.size() > NUM_IMAGE_POSITIONS) {
    images_dq.pop_front();
    keypoints_dq.pop_front();
    descriptors_dq.pop_front();
    if (!bin_slots_dq_.empty()) bin_slots_dq_.pop_front();
  }
}

// The resident protocol, once: a stereo pair through ONE call of its route into the next slot pair of the ring of four; the deques are filled
// from what the call hands out, which is what detectKeypoints + describeKeypoints produce image by image.  Features: the route's
// spvo_*_features (its record type and its rows' element type); call(slot_l, slot_r, f): the library call.  false: nothing was pushed.
template <class Features, class Call>
bool ClassicFeatureFrontEnd::residentPair(const ClassicPair &p, cv::Mat &img_l, cv::Mat &img_r, const char *name, Call call) {
  using Record = typename std::remove_pointer<decltype(Features::kp)>::type;
  using Element = typename std::remove_pointer<decltype(Features::desc)>::type;
  // the two standard matches go out with the detector from now on
  if (resident_pairs_ == 0) {
    spvo_set_prematch(ctx_, 1, selector_type_ == SelectorType::KNN ? SPVO_SELECT_KNN : SPVO_SELECT_NN, matcher_cross_check_ ? 1 : 0, knn_threshold_);
    if (matcher_flann_) spvo_set_binary_prematch_norm(ctx_, SPVO_NORM_L2);   // (the SIFT slots' prematch is L2 either way)
  }
  const int cap = std::max(resident_capacity_, 1);
  Features f[2];
  for (int k = 0; k < 2; ++k) {
    Staging &s = staging_[k];
    if (s.records.size() != (size_t)cap * sizeof(Record)) { s.records.resize((size_t)cap * sizeof(Record)); s.rows.resize((size_t)cap * p.rowBytes()); }   // first pair only
    f[k] = Features{0, reinterpret_cast<Record *>(s.records.data()), reinterpret_cast<Element *>(s.rows.data()), cap};
  }
  const int slot_l = 2 * (int)(resident_pairs_ % 4), slots[2] = {slot_l, slot_l + 1};
  ++resident_pairs_;   // counts attempts: a failed call has used its slot pair
  const int rc = call(slots[0], slots[1], f);
  if (rc != SPVO_OK) {   // SPVO_ERR_CAPACITY: the pair does not fit its slots; anything else is reported -- the per-image path follows either way
    if (rc != SPVO_ERR_CAPACITY) logError(std::string(name) + ": " + spvo_last_error(ctx_));
    return false;
  }
  ++resident_ok_pairs_;
  cv::Mat *imgs[2] = {&img_l, &img_r};
  for (int k = 0; k < 2; ++k) {
    images_dq.push_back(*imgs[k]);
    keypoints_dq.push_back(to_keypoints(f[k].kp, f[k].n, p, true));
    descriptors_dq.push_back(copy_rows(f[k].desc, f[k].n, p));
    bin_slots_dq_.push_back(slots[k]);
  }
  return true;
}

// is level `octave` of spvo_orb_describe_octaves' pyramid (scale 1.2 per level, sizes rounded) at least the 32 x 32 the extractor accepts?
static bool orb_level_ok(int rows, int cols, int octave) {
  float scale = 1.f;
  for (int l = 0; l < octave; ++l) scale *= 1.2f;
  return std::lround(rows / scale) >= 32 && std::lround(cols / scale) >= 32;
}

// setDeviceResident: the pair through its route (residentPair).  false: nothing was pushed and the caller takes the per-image path -- the pair
// has no route or lacks its opt-in (residentPairs() stays 0), it does not fit its slots, or the call failed and the per-image path reports why.
bool ClassicFeatureFrontEnd::addStereoImagePairResident(cv::Mat &img_l, cv::Mat &img_r) {
  if (!image_ok(img_l) || !image_ok(img_r) || (size_t)img_l.step != (size_t)img_r.step) return false;
  const ClassicPair &p = *pair();   // (addStereoImagePair has asked pairRuns)
  if (p.route == Route::None || (p.resident_opt_in == OptIn::BriskPairResident && !brisk_pair_resident_) || (p.resident_opt_in == OptIn::AkazePairResident && !akaze_pair_resident_) ||
      (p.resident_opt_in == OptIn::SiftDescribeResident && !sift_describe_resident_) || (p.resident_opt_in == OptIn::OctavePairsResident && !octave_pairs_resident_) ||
      (p.resident_opt_in == OptIn::SiftOctavePairsResident && !sift_octave_pairs_resident_) || (p.resident_opt_in == OptIn::OrbPairsResident && !orb_pairs_resident_) ||
      (p.resident_opt_in == OptIn::SiftBriskResident && !sift_brisk_resident_))
    return false;
  const uint8_t *l = img_l.ptr<uint8_t>(0), *r = img_r.ptr<uint8_t>(0);
  const int rows = img_l.rows, cols = img_l.cols;
  const size_t step = (size_t)img_l.step;
  switch (p.route) {
  case Route::Classic: {
    spvo_classic_opts opts;
    spvo_default_classic_opts(&opts, p.kind);
    opts.slot_capacity = resident_capacity_;
    return residentPair<spvo_classic_features>(p, img_l, img_r, "spvo_classic_detect", [&](int slot_l, int slot_r, spvo_classic_features *f) {
      return spvo_classic_detect(ctx_, &opts, l, r, rows, cols, step, slot_l, slot_r, &f[0], &f[1]);
    });
  }
  case Route::SiftPair:
    return residentPair<spvo_sift_features>(p, img_l, img_r, "spvo_sift_detect_pair", [&](int slot_l, int slot_r, spvo_sift_features *f) {
      return spvo_sift_detect_pair(ctx_, l, r, rows, cols, step, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::BriskPair:   // cv::BRISK::create(): threshold 30, 3 octaves, as detectKeypoints
    return residentPair<spvo_brisk_features>(p, img_l, img_r, "spvo_brisk_detect_pair", [&](int slot_l, int slot_r, spvo_brisk_features *f) {
      return spvo_brisk_detect_pair(ctx_, l, r, rows, cols, step, 30, 3, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::AkazePair:   // cv::AKAZE::create(): threshold 0.001, as detectKeypoints
    return residentPair<spvo_akaze_features>(p, img_l, img_r, "spvo_akaze_detect_pair", [&](int slot_l, int slot_r, spvo_akaze_features *f) {
      return spvo_akaze_detect_pair(ctx_, l, r, rows, cols, step, 0.001f, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::ClassicSift: {   // the detector's parameters are detectKeypoints': spvo_default_classic_opts
    spvo_classic_opts opts;
    spvo_default_classic_opts(&opts, p.kind);
    opts.slot_capacity = resident_capacity_;
    return residentPair<spvo_sift_features>(p, img_l, img_r, "spvo_classic_sift_pair", [&](int slot_l, int slot_r, spvo_sift_features *f) {
      return spvo_classic_sift_pair(ctx_, &opts, l, r, rows, cols, step, slot_l, slot_r, &f[0], &f[1]);
    });
  }
  // The ORB pairs refuse a shape whose pyramid level at the detector's highest octave (BRISK: layer 5; AKAZE: the octave of the shape's last
  // level) is smaller than 32 x 32, where the per-image path asks only about the levels its keypoints name: such a shape takes that path, uncounted
  case Route::BriskOrbPair:
    if (!orb_level_ok(rows, cols, 5)) return false;
    return residentPair<spvo_brisk_features>(p, img_l, img_r, "spvo_brisk_orb_pair", [&](int slot_l, int slot_r, spvo_brisk_features *f) {
      return spvo_brisk_orb_pair(ctx_, l, r, rows, cols, step, 30, 3, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::AkazeOrbPair: {
    int levels = 0, n_tau = 0;
    int32_t octave[16] = {0};
    if (rows < 16 || cols < 16 || spvo_akaze_tables(rows, cols, &levels, octave, nullptr, nullptr, nullptr, nullptr, 0, &n_tau, nullptr, nullptr) != SPVO_OK || levels < 1 ||
        !orb_level_ok(rows, cols, octave[levels - 1]))
      return false;
    return residentPair<spvo_akaze_features>(p, img_l, img_r, "spvo_akaze_orb_pair", [&](int slot_l, int slot_r, spvo_akaze_features *f) {
      return spvo_akaze_orb_pair(ctx_, l, r, rows, cols, step, 0.001f, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  }
  case Route::AkazeBriskPair:
    return residentPair<spvo_akaze_features>(p, img_l, img_r, "spvo_akaze_brisk_pair", [&](int slot_l, int slot_r, spvo_akaze_features *f) {
      return spvo_akaze_brisk_pair(ctx_, l, r, rows, cols, step, 0.001f, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  // The SIFT pairs build the extractor's pyramid up to the detector's highest octave (BRISK: 5; AKAZE: that of the shape's last level) and
  // refuse a shape without that octave, where the per-image path asks only about the octaves its keypoints name: such a shape takes that
  // path, uncounted (the orb_level_ok precedent)
  case Route::BriskSiftPair:
    if ((std::min(rows, cols) >> 5) < 1) return false;
    return residentPair<spvo_sift_features>(p, img_l, img_r, "spvo_brisk_sift_pair", [&](int slot_l, int slot_r, spvo_sift_features *f) {
      return spvo_brisk_sift_pair(ctx_, l, r, rows, cols, step, 30, 3, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::AkazeSiftPair: {
    int levels = 0, n_tau = 0;
    int32_t octave[16] = {0};
    if (rows < 16 || cols < 16 || spvo_akaze_tables(rows, cols, &levels, octave, nullptr, nullptr, nullptr, nullptr, 0, &n_tau, nullptr, nullptr) != SPVO_OK || levels < 1 ||
        (std::min(rows, cols) >> octave[levels - 1]) < 1)
      return false;
    return residentPair<spvo_akaze_sift_features>(p, img_l, img_r, "spvo_akaze_sift_pair", [&](int slot_l, int slot_r, spvo_akaze_sift_features *f) {
      return spvo_akaze_sift_pair(ctx_, l, r, rows, cols, step, 0.001f, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  }
  // cv::ORB::create(2000, ..), as detectKeypoints.  No shape is refused that the per-image path accepts: the pyramid is built up to the
  // highest level that can hold a keypoint, and SIFT's octave of that number exists for every such shape
  case Route::OrbBriskPair:
    return residentPair<spvo_brisk_features>(p, img_l, img_r, "spvo_orb_brisk_pair", [&](int slot_l, int slot_r, spvo_brisk_features *f) {
      return spvo_orb_brisk_pair(ctx_, l, r, rows, cols, step, 2000, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::OrbSiftPair:
    return residentPair<spvo_sift_features>(p, img_l, img_r, "spvo_orb_sift_pair", [&](int slot_l, int slot_r, spvo_sift_features *f) {
      return spvo_orb_sift_pair(ctx_, l, r, rows, cols, step, 2000, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  // cv::SIFT::create(), as detectKeypoints; no shape is refused that the per-image path accepts
  case Route::SiftBriskPair:
    return residentPair<spvo_brisk_features>(p, img_l, img_r, "spvo_sift_brisk_pair", [&](int slot_l, int slot_r, spvo_brisk_features *f) {
      return spvo_sift_brisk_pair(ctx_, l, r, rows, cols, step, slot_l, slot_r, resident_capacity_, &f[0], &f[1]);
    });
  case Route::None:
    break;
  }
  return false;
}
#endif

// The reference's constructor hands `stereo_threshold` to the base class a second time in the place of `min_disparity`
// (hpp:203-206), so the classic launch file's min_disparity is never used; kept, because the stereo gate of
// solveStereoOdometry (base.cpp:169-172) then behaves as the reference's does.
ClassicFeatureFrontEnd::ClassicFeatureFrontEnd()
    : ClassicFeatureFrontEnd(DetectorType::ShiTomasi, DescriptorType::ORB, MatcherType::BF, SelectorType::NN, true, 2.0f, 1.0f, 4, true, 120, 392) {}

ClassicFeatureFrontEnd::ClassicFeatureFrontEnd(const DetectorType detector_type, const DescriptorType descriptor_type, const MatcherType matcher_type,
                                               const SelectorType selector_type, const bool cross_check, const float stereo_threshold,
                                               const float /*min_disparity*/, const int refinement_degree, const bool verbose, const int input_height,
                                               const int input_width)
    : FeatureFrontEnd(detector_type, descriptor_type, matcher_type, selector_type, cross_check, stereo_threshold, stereo_threshold, refinement_degree,
                      verbose, input_height, input_width) {
  akaze_descriptor_ = g_classic_akaze_descriptor;   // (initDetector and initDescriptor ask whether the pair runs)
  orb_octaves_ = g_classic_orb_octaves;
  orb_brisk_ = g_classic_orb_brisk;
  sift_brisk_ = g_classic_sift_brisk;
  initDetector();
  initDescriptor();
  initMatcher();
#ifndef SPVO_USE_OPENCV
  if (const ClassicPair *p = pair()) matcher_hamming_ = p->type == CV_8UC1;   // the norm goes with the row's element type
#endif
  resident_ = g_classic_resident;
  resident_capacity_ = g_classic_resident_capacity;
  brisk_pair_resident_ = g_classic_brisk_pair_resident;
  akaze_pair_resident_ = g_classic_akaze_pair_resident;
  sift_describe_resident_ = g_classic_sift_describe_resident;
  octave_pairs_resident_ = g_classic_octave_pairs_resident;
  sift_octave_pairs_resident_ = g_classic_sift_octave_pairs_resident;
  orb_pairs_resident_ = g_classic_orb_pairs_resident;
  sift_brisk_resident_ = g_classic_sift_brisk_resident;
}

ClassicFeatureFrontEnd::~ClassicFeatureFrontEnd() {
  if (ctx_) spvo_destroy(ctx_);
  ctx_ = nullptr;
}
