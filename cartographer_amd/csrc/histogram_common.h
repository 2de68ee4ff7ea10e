// What the single histogram (filters.hip: cmx_compute_histogram) and the batched one
// (histogram_batch.hip: cmx_compute_histogram_batch) have in common: the constants of
// RotationalScanMatcher (rotational_scan_matcher.cc:30-33) and the two squared thresholds the
// host hands to the walk.  Plain C++.
#ifndef CMX_HISTOGRAM_COMMON_H_
#define CMX_HISTOGRAM_COMMON_H_
#include <cmath>

namespace cmx {

constexpr float kMinDistance = 0.2f, kMaxDistance = 0.9f, kSliceHeight = 0.2f;
constexpr unsigned kNoVote = 0xffffu;      // bucket key of a point without a vote (> any bucket)

// distance < kMin <=> d2 < min_sq, distance > kMax <=> d2 > max_sq for the correctly rounded
// f32 square root of the reference (monotone): the smallest d2 whose root reaches kMin, the
// largest whose root does not exceed kMax.
inline float HistogramMinDistanceSq() {
  static const float min_sq = [] {
    float x = kMinDistance * kMinDistance;
    while (std::sqrt(x) >= kMinDistance) x = std::nextafter(x, 0.f);
    while (std::sqrt(x) < kMinDistance) x = std::nextafter(x, 1.f);
    return x;
  }();
  return min_sq;
}
inline float HistogramMaxDistanceSq() {
  static const float max_sq = [] {
    float x = kMaxDistance * kMaxDistance;
    while (std::sqrt(x) <= kMaxDistance) x = std::nextafter(x, 2.f);
    while (std::sqrt(x) > kMaxDistance) x = std::nextafter(x, 0.f);
    return x;
  }();
  return max_sq;
}

}  // namespace cmx
#endif  // CMX_HISTOGRAM_COMMON_H_
