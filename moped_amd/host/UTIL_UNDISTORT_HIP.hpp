// UTIL_UNDISTORT_HIP -- drop-in for UTIL_UNDISTORT (src/util/UTIL_UNDISTORT.hpp), the first step of both default
// pipelines (moped2 config.hpp:59, moped3d config.hpp:38).  Wire it BEFORE the CPU step under the same step name:
//     pipeline.addAlg( "UNDISTORTED_IMAGE", new UTIL_UNDISTORT_HIP );
//     pipeline.addAlg( "UNDISTORTED_IMAGE", new UTIL_UNDISTORT );   // fallback (needs OpenCV)
// Contract kept (:102-135): every image of the frame is resampled in place, its first width x height bytes, with the
// maps of its own (width, height, intrinsicLinearCalibration, intrinsicNonlinearCalibration); the maps are built once
// per camera and kept (the library keeps the last MH_MAX_IMAGES cameras of its context).  Images whose data is
// shorter than width x height are left alone.  Under MOPED_AMD_WITH_DEPTH only gray images are resampled: the
// reference also runs the remap over the first width x height bytes of a depth map's floats, which this step does
// not reproduce.
#pragma once
#include "hip_session.hpp"

namespace MopedNS {

class UTIL_UNDISTORT_HIP : public MopedAlg {
 public:
  UTIL_UNDISTORT_HIP() { capable = HipSession::get() != 0; }

  void process(FrameData& frameData) {
    mh_ctx* ctx = HipSession::get();
    for (int i = 0; i < (int)frameData.images.size(); i++) {
      Image* image = frameData.images[i].get();
#ifdef MOPED_AMD_WITH_DEPTH
      if (image->imageType != IMAGE_TYPE_GRAY_IMAGE) continue;
#endif
      if (image->width <= 0 || image->height <= 0 || (int)image->data.size() < image->width * image->height) continue;
      float K[4], dist[4];
      for (int k = 0; k < 4; k++) {
        K[k] = image->intrinsicLinearCalibration[k];      // fx, fy, cx, cy (:77-81)
        dist[k] = image->intrinsicNonlinearCalibration[k];   // k1, k2, p1, p2 (:84-87)
      }
      if (mh_undistort(ctx, &image->data[0], &image->data[0], image->width, image->height, K, dist) != MH_OK)
        HipSession::warn("mh_undistort");
    }
  }
};

}  // namespace MopedNS
