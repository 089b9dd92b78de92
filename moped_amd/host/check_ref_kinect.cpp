// createModelFromKinectViews_HIP and createMergedModelFromKinectViews_HIP compiled against the reference's REAL
// include/moped.hpp (`make check_ref_kinect`), at the reference's language level: SP_Image, SP_Model, Pose and Float are
// then the reference's own.  Only src/util.hpp's part comes from the mirror (util.hpp needs OpenCV).  Syntax only; skipped
// where the reference is absent.
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <moped.hpp>
namespace std { using tr1::shared_ptr; }
#include "moped_util_mirror.hpp"
#include "kinect_models_hip.hpp"

int main() {
  std::vector<MopedNS::SP_Image> images, depthmaps;
  std::vector<MopedNS::Pose> poses;
  std::vector<int> views;
  int index = 0;
  // no session: an empty result, nothing touched
  if (MopedNS::createModelFromKinectViews_HIP(0, "m", images, depthmaps, poses, &index)) return 1;
  if (MopedNS::createMergedModelFromKinectViews_HIP(0, "m", images, depthmaps, poses, 2, &index, &views)) return 1;
  return 0;
}
