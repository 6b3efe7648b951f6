// What other translation units may ask of a plvs_stereo (stereo.hip).
#pragma once
#include "../../include/plvs_hip.h"

namespace plvs {
// true when `s` was created by plvs_hip_stereo_create(left, right, ...): its matches read these two extractors' pyramids
bool stereo_made_from(const plvs_stereo* s, const plvs_orb* left, const plvs_orb* right);
}  // namespace plvs
