// The reference's own Frame::isInFrustum(MapPointPtr&, float) / (MapLinePtr&, float), the PredictScale(const float&, Frame*) of
// MapPoint and MapLine, the four Get{Min,Max}DistanceInvariance and Pinhole::project(const Eigen::Vector3f&), behind a C
// interface.  This file holds declarations and calls only: the DEFINITIONS are cut verbatim out of the reference tree into
// track_local_cut.inc at build time (scripts/make_track_local_golden.py) and compiled here, against oracle/ref/eigen_full,
// with -O2 -ffp-contract=off -fno-fast-math.  The classes below carry exactly the members those definitions touch — not
// oracle/ref/slam_shim/slam_shim_map.h, whose PredictScale aborts and whose MapLine::GetMinDistanceInvariance differs from
// the reference's.
#include <cmath>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include <Eigen/Core>

using namespace std;   // in effect in the original units: log(float) below is std::log(float)

namespace PLVS2 {

class Frame;
class KeyFrame;
typedef KeyFrame* KeyFramePtr;

class Pinhole {
 public:
  Eigen::Vector2f project(const Eigen::Vector3f& v3D) const;
  std::vector<float> mvParameters;
};

class MapPoint {
 public:
  Eigen::Vector3f GetWorldPos() { return mWorldPos; }
  Eigen::Vector3f GetNormal() { return mNormalVector; }
  float GetMinDistanceInvariance();
  float GetMaxDistanceInvariance();
  int PredictScale(const float& currentDist, Frame* pF);
  bool mbTrackInView = false, mbTrackInViewR = false;
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackDepth = 0, mTrackViewCos = 0;
  int mnTrackScaleLevel = 0, mnTrackScaleLevelR = 0;
  Eigen::Vector3f mWorldPos, mNormalVector;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexPos;
};
typedef MapPoint* MapPointPtr;

class MapLine {
 public:
  void GetWorldEndPoints(Eigen::Vector3f& s, Eigen::Vector3f& e) { s = mWorldPosStart; e = mWorldPosEnd; }
  Eigen::Vector3f GetNormal() { return mNormalVector; }
  float GetMinDistanceInvariance();
  float GetMaxDistanceInvariance();
  int PredictScale(const float& currentDist, Frame* pF);
  bool mbTrackInView = false, mbTrackInViewR = false;
  float mTrackProjStartX = 0, mTrackProjStartY = 0, mTrackProjStartXR = 0, mTrackProjStartYR = 0;
  float mTrackProjEndX = 0, mTrackProjEndY = 0, mTrackProjEndXR = 0, mTrackProjEndYR = 0;
  float mTrackStartDepth = 0, mTrackEndDepth = 0, mTrackViewCos = 0;
  int mnTrackScaleLevel = 0, mnTrackScaleLevelR = 0;
  Eigen::Vector3f mWorldPosStart, mWorldPosEnd, mNormalVector;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexPos;
};
typedef MapLine* MapLinePtr;

class Frame {
 public:
  bool isInFrustum(MapPointPtr& pMP, float viewingCosLimit);
  bool isInFrustum(MapLinePtr& pML, float viewingCosLimit);
  // the two-camera branches are never taken here (Nleft == NlinesLeft == -1)
  bool isInFrustumChecks(MapPointPtr, float, bool = false) { abort(); }
  bool isInFrustumChecks(MapLinePtr, float, bool = false) { abort(); }
  int Nleft = -1, NlinesLeft = -1;
  Pinhole* mpCamera = nullptr;
  Eigen::Matrix3f mRcw;
  Eigen::Vector3f mtcw, mOw;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mbf = 0;
  float mfLogScaleFactor = 0, mfLineLogScaleFactor = 0;
  int mnScaleLevels = 0, mnLineScaleLevels = 0;
};

#include "track_local_cut.inc"

}  // namespace PLVS2

namespace {

void fill(PLVS2::Frame& F, PLVS2::Pinhole& cam, const float* K4, float mbf, const float* bounds4, const float* Rcw, const float* tcw,
          const float* Ow, float lsf, int levels, float line_lsf, int line_levels) {
  cam.mvParameters.assign(K4, K4 + 4);
  F.mpCamera = &cam;
  for (int i = 0; i < 9; ++i) F.mRcw(i) = Rcw[i];   // the layout Eigen::Matrix3f has in memory
  for (int i = 0; i < 3; ++i) { F.mtcw(i) = tcw[i]; F.mOw(i) = Ow[i]; }
  F.mnMinX = bounds4[0]; F.mnMaxX = bounds4[1]; F.mnMinY = bounds4[2]; F.mnMaxY = bounds4[3];
  F.mbf = mbf;
  F.mfLogScaleFactor = lsf; F.mnScaleLevels = levels;
  F.mfLineLogScaleFactor = line_lsf; F.mnLineScaleLevels = line_levels;
}

}  // namespace

extern "C" {

// The loop of Tracking::SearchLocalPoints over the map points that are not skipped: -> nToMatch.  Skipped elements keep the
// values the arrays come in with.
int ref_is_in_frustum_points(const float* K4, float mbf, const float* bounds4, const float* Rcw, const float* tcw, const float* Ow,
                             float viewing_cos_limit, float lsf, int levels, int m, const uint8_t* skip, const float* pos,
                             const float* normal, const float* min_dist, const float* max_dist, uint8_t* in_view, float* proj_x,
                             float* proj_y, float* proj_xr, float* track_depth, int32_t* level, float* view_cos) {
  PLVS2::Frame F;
  PLVS2::Pinhole cam;
  fill(F, cam, K4, mbf, bounds4, Rcw, tcw, Ow, lsf, levels, lsf, levels);
  int n = 0;
  for (int k = 0; k < m; ++k) {
    if (skip[k]) continue;
    PLVS2::MapPoint mp;
    mp.mWorldPos = Eigen::Vector3f(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
    mp.mNormalVector = Eigen::Vector3f(normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]);
    mp.mfMinDistance = min_dist[k];
    mp.mfMaxDistance = max_dist[k];
    mp.mTrackProjXR = proj_xr[k]; mp.mTrackDepth = track_depth[k]; mp.mnTrackScaleLevel = level[k]; mp.mTrackViewCos = view_cos[k];
    PLVS2::MapPointPtr p = &mp;
    if (F.isInFrustum(p, viewing_cos_limit)) ++n;
    in_view[k] = mp.mbTrackInView;
    proj_x[k] = mp.mTrackProjX; proj_y[k] = mp.mTrackProjY; proj_xr[k] = mp.mTrackProjXR;
    track_depth[k] = mp.mTrackDepth; level[k] = mp.mnTrackScaleLevel; view_cos[k] = mp.mTrackViewCos;
  }
  return n;
}

// The loop of Tracking::SearchLocalLines.  proj: 6 per line (StartX, StartY, EndX, EndY, mTrackStartDepth, mTrackEndDepth),
// proj_xr: 2 per line (mTrackProjStartXR, mTrackProjEndXR).
int ref_is_in_frustum_lines(const float* K4, float mbf, const float* bounds4, const float* Rcw, const float* tcw, const float* Ow,
                            float viewing_cos_limit, float line_lsf, int line_levels, int m, const uint8_t* skip, const float* start,
                            const float* end, const float* normal, const float* max_dist, uint8_t* in_view, float* proj, float* proj_xr,
                            int32_t* level, float* view_cos) {
  PLVS2::Frame F;
  PLVS2::Pinhole cam;
  fill(F, cam, K4, mbf, bounds4, Rcw, tcw, Ow, line_lsf, line_levels, line_lsf, line_levels);
  int n = 0;
  for (int k = 0; k < m; ++k) {
    if (skip[k]) continue;
    PLVS2::MapLine ml;
    ml.mWorldPosStart = Eigen::Vector3f(start[3 * k], start[3 * k + 1], start[3 * k + 2]);
    ml.mWorldPosEnd = Eigen::Vector3f(end[3 * k], end[3 * k + 1], end[3 * k + 2]);
    ml.mNormalVector = Eigen::Vector3f(normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]);
    ml.mfMinDistance = 0.0f;   // (never read: the reference's band is [0.8f, 1.2f] * mfMaxDistance)
    ml.mfMaxDistance = max_dist[k];
    ml.mTrackStartDepth = proj[6 * k + 4]; ml.mTrackEndDepth = proj[6 * k + 5];
    ml.mnTrackScaleLevel = level[k]; ml.mTrackViewCos = view_cos[k];
    PLVS2::MapLinePtr p = &ml;
    if (F.isInFrustum(p, viewing_cos_limit)) ++n;
    in_view[k] = ml.mbTrackInView;
    proj[6 * k] = ml.mTrackProjStartX; proj[6 * k + 1] = ml.mTrackProjStartY;
    proj[6 * k + 2] = ml.mTrackProjEndX; proj[6 * k + 3] = ml.mTrackProjEndY;
    proj[6 * k + 4] = ml.mTrackStartDepth; proj[6 * k + 5] = ml.mTrackEndDepth;
    proj_xr[2 * k] = ml.mTrackProjStartXR; proj_xr[2 * k + 1] = ml.mTrackProjEndXR;
    level[k] = ml.mnTrackScaleLevel; view_cos[k] = ml.mTrackViewCos;
  }
  return n;
}

// PredictScale alone (the level rule's tests): kind 0 = MapPoint, 1 = MapLine
int ref_predict_scale(int kind, float max_dist, float dist, float lsf, int levels) {
  PLVS2::Frame F;
  F.mfLogScaleFactor = F.mfLineLogScaleFactor = lsf;
  F.mnScaleLevels = F.mnLineScaleLevels = levels;
  if (kind == 0) {
    PLVS2::MapPoint mp;
    mp.mfMaxDistance = max_dist;
    return mp.PredictScale(dist, &F);
  }
  PLVS2::MapLine ml;
  ml.mfMaxDistance = max_dist;
  return ml.PredictScale(dist, &F);
}

}  // extern "C"
