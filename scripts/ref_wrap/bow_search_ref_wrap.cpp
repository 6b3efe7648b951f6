// Wrapper of ours around the reference's two ORBmatcher::SearchByBoW definitions, ORBmatcher::ComputeThreeMaxima,
// ORBmatcher::DescriptorDistance and the matcher's constants, which scripts/make_bow_search_golden.py cuts verbatim out of the
// reference tree into bow_search_cut_*.inc next to this file's build at build time (no cut text is kept).  Everything here is a
// stand-in the cut text compiles against: the objects hold what the scenario gives them, and the accessors the compiled text calls
// record what it did — the distances it took per serial feature (cv::Mat::ptr), and the bin it pushed a match into (its own call of
// round, seen through a macro).
#include <assert.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <map>
#include <vector>

namespace obs {
static int* n_dist = nullptr;     // per serial feature: distances taken
static int* bin_of = nullptr;     // per serial feature: round(rot * factor) as the cut computed it (before bin == HISTO_LENGTH -> 0), else -1
static int current = -1;          // the serial feature whose descriptor was read last
static int reads = 0;
inline float seen_round(float x) {
  const float r = std::round(x);
  if (bin_of && current >= 0) bin_of[current] = (int)r;
  return r;
}
inline double seen_round(double x) {
  const double r = std::round(x);
  if (bin_of && current >= 0) bin_of[current] = (int)r;
  return r;
}
}  // namespace obs

namespace cv {
struct KeyPoint {
  float angle;
};
struct Mat {
  const uint8_t* data = nullptr;
  int index = -1;       // the row this is
  bool serial = false;  // a row of the side the cut walks in its outer loop
  Mat row(int i) const {
    Mat m;
    m.data = data + 32 * (size_t)i;
    m.index = i;
    m.serial = serial;
    return m;
  }
  template <class T>
  const T* ptr() const {
    if (serial) obs::current = index;
    if (++obs::reads % 2 == 0 && obs::n_dist && obs::current >= 0) ++obs::n_dist[obs::current];
    return reinterpret_cast<const T*>(data);
  }
};
}  // namespace cv

namespace DBoW2 {
typedef std::map<unsigned int, std::vector<unsigned int> > FeatureVector;
}

using namespace std;

namespace PLVS2 {

struct MapPoint {
  bool bad = false;
  bool isBad() const { return bad; }
};
typedef MapPoint* MapPointPtr;

struct KeyFrame {
  int NLeft = -1;
  void* mpCamera2 = nullptr;
  std::vector<cv::KeyPoint> mvKeysUn, mvKeys, mvKeysRight;
  cv::Mat mDescriptors;
  DBoW2::FeatureVector mFeatVec;
  std::vector<MapPointPtr> points;
  std::vector<MapPointPtr> GetMapPointMatches() const { return points; }
};
typedef KeyFrame* KeyFramePtr;

struct Frame {
  int N = 0, Nleft = -1;
  void* mpCamera2 = nullptr;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
  cv::Mat mDescriptors;
  DBoW2::FeatureVector mFeatVec;
};

class ORBmatcher {
 public:
  ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b);
  int SearchByBoW(KeyFramePtr& pKF, Frame& F, std::vector<MapPointPtr>& vpMapPointMatches);
  int SearchByBoW(KeyFramePtr& pKF1, KeyFramePtr& pKF2, std::vector<MapPointPtr>& vpMatches12);
  static const int TH_LOW;
  static const int TH_HIGH;
  static const int HISTO_LENGTH;

 protected:
  void ComputeThreeMaxima(std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3);
  float mfNNratio;
  bool mbCheckOrientation;
};

}  // namespace PLVS2

#include "bow_search_cut_define.inc"
namespace PLVS2 {
#include "bow_search_cut_constants.inc"
#define round(x) obs::seen_round(x)
#include "bow_search_cut_defs.inc"
#undef round
#include "bow_search_cut_helpers.inc"
}  // namespace PLVS2

namespace {

struct Side {
  std::vector<PLVS2::MapPoint> points;   // one per feature; valid[i] == 0: a null pointer
  DBoW2::FeatureVector vec;
  std::vector<cv::KeyPoint> keys;
  std::vector<PLVS2::MapPointPtr> ptrs;
  const uint8_t* desc;
  Side(int n, const uint8_t* desc_, const float* angle, const uint8_t* valid, int nnodes, const uint32_t* node_id, const int32_t* off,
       const uint32_t* idx)
      : points((size_t)n), keys((size_t)n), ptrs((size_t)n, nullptr), desc(desc_) {
    for (int i = 0; i < n; ++i) {
      keys[i].angle = angle[i];
      if (!valid || valid[i] == 1) ptrs[i] = &points[i];
      if (valid && valid[i] == 2) { ptrs[i] = &points[i]; points[i].bad = true; }   // a bad map point: the other way to fail the gate
    }
    for (int a = 0; a < nnodes; ++a) {
      std::vector<unsigned int>& list = vec[node_id[a]];
      for (int p = off[a]; p < off[a + 1]; ++p) list.push_back(idx[p]);
    }
  }
  void fill(PLVS2::KeyFrame* kf, bool serial) const {
    kf->mvKeysUn = keys;
    kf->mDescriptors.data = desc;
    kf->mDescriptors.serial = serial;
    kf->mFeatVec = vec;
    kf->points = ptrs;
  }
};

}  // namespace

extern "C" {

int ref_th_low() { return PLVS2::ORBmatcher::TH_LOW; }
int ref_histo_length() { return PLVS2::ORBmatcher::HISTO_LENGTH; }

// valid: 0 null, 1 good, 2 bad.  match12[i1]: the key point of key frame 2 whose map point vpMatches12[i1] holds, else -1.
int ref_bow_kf_kf(int n1, const uint8_t* desc1, const float* angle1, const uint8_t* valid1, int nn1, const uint32_t* id1, const int32_t* off1,
                  const uint32_t* idx1, int n2, const uint8_t* desc2, const float* angle2, const uint8_t* valid2, int nn2, const uint32_t* id2,
                  const int32_t* off2, const uint32_t* idx2, float nn_ratio, int check_orientation, int32_t* match12, int* n_dist, int* bin_of) {
  const Side s1(n1, desc1, angle1, valid1, nn1, id1, off1, idx1), s2(n2, desc2, angle2, valid2, nn2, id2, off2, idx2);
  PLVS2::KeyFrame kf1, kf2;
  s1.fill(&kf1, true);
  s2.fill(&kf2, false);
  PLVS2::KeyFramePtr p1 = &kf1, p2 = &kf2;
  obs::n_dist = n_dist; obs::bin_of = bin_of; obs::current = -1; obs::reads = 0;
  for (int i = 0; n_dist && i < n1; ++i) { n_dist[i] = 0; bin_of[i] = -1; }
  std::vector<PLVS2::MapPointPtr> matches;
  PLVS2::ORBmatcher matcher(nn_ratio, check_orientation != 0);
  const int n = matcher.SearchByBoW(p1, p2, matches);
  obs::n_dist = obs::bin_of = nullptr;
  for (int i = 0; match12 && i < n1; ++i) match12[i] = matches[i] ? (int)(matches[i] - s2.points.data()) : -1;
  return n;
}

// assigned[iF]: the key point of the key frame whose map point vpMapPointMatches[iF] holds, else -1
int ref_bow_kf_frame(int nk, const uint8_t* desck, const float* anglek, const uint8_t* validk, int nnk, const uint32_t* idk, const int32_t* offk,
                     const uint32_t* idxk, int nf, const uint8_t* descf, const float* anglef, int nnf, const uint32_t* idf, const int32_t* offf,
                     const uint32_t* idxf, float nn_ratio, int check_orientation, int32_t* assigned, int* n_dist, int* bin_of) {
  const Side sk(nk, desck, anglek, validk, nnk, idk, offk, idxk), sf(nf, descf, anglef, nullptr, nnf, idf, offf, idxf);
  PLVS2::KeyFrame kf;
  sk.fill(&kf, true);
  PLVS2::Frame F;
  F.N = nf;
  F.mvKeys = sf.keys;
  F.mDescriptors.data = descf;
  F.mFeatVec = sf.vec;
  PLVS2::KeyFramePtr pk = &kf;
  obs::n_dist = n_dist; obs::bin_of = bin_of; obs::current = -1; obs::reads = 0;
  for (int i = 0; n_dist && i < nk; ++i) { n_dist[i] = 0; bin_of[i] = -1; }
  std::vector<PLVS2::MapPointPtr> matches;
  PLVS2::ORBmatcher matcher(nn_ratio, check_orientation != 0);
  const int n = matcher.SearchByBoW(pk, F, matches);
  obs::n_dist = obs::bin_of = nullptr;
  for (int i = 0; assigned && i < nf; ++i) assigned[i] = matches[i] ? (int)(matches[i] - sk.points.data()) : -1;
  return n;
}

}  // extern "C"
