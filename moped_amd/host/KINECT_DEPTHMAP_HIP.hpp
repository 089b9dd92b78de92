// KINECT_DEPTHMAP_HIP -- the depth map of a Kinect frame from what the sensor delivers, built on the device: the
// replacement for the block of moped3d's ROS node between the gray image and processImages (moped3d/moped3d.cpp:270-333).
// It is no STEP: the reference has none here, the node builds the map before the pipeline sees the frame.  In the node,
//
//     SP_Image depthmap( new Image );
//     mh_raw_depth raw = hipRawDepthOfCloud( pMsg->width, pMsg->height, pMsg->point_step, pMsg->row_step, 8 );
//     if( !hipKinectDepthmap( *depthmap, &pMsg->data[0], raw, DepthIntrinsicLinearCalibration,
//                             DepthIntrinsicNonlinearCalibration, gs.width, gs.height ) ) { ... the node's own loop ... }
//     images.push_back( depthmap );
//
// replaces :270-333: the cloud is read in place (its z field at byte 8 of every point, NaN = no reading), 1.2 MB go to the
// device instead of a 307 200-pixel host loop, the finished [height][width][4] map comes back into depthmap->data.  OpenNI's
// 16-bit millimetre image (0 = no reading) goes the same way with hipRawDepthOfImage16.  A raw buffer of another size than
// the gray image is resized to twice its size as the node does (:303); the resize restates cv::resize from memory and is
// unpinned (csrc/depthmap.hip).  The nonlinear coefficients are stored and never applied, as in the node.
// Needs moped3d's Image (MOPED_AMD_WITH_DEPTH with moped_types.hpp); Float must be float, as everywhere in the plugins.
#pragma once
#include "hip_session.hpp"

namespace MopedNS {

// an organised PointCloud2: `width` x `height` points of point_step bytes, rows of row_step bytes, float z at zOffset
inline mh_raw_depth hipRawDepthOfCloud(int width, int height, int pointStep, int rowStep, int zOffset) {
  mh_raw_depth r;
  r.format = MH_RAW_DEPTH_F32_M;
  r.width = width;
  r.height = height;
  r.elem_stride = pointStep;
  r.row_stride = rowStep;
  r.offset = zOffset;
  return r;
}
// a plain float image in metres (NaN = no reading), rows of rowStep bytes (0: packed)
inline mh_raw_depth hipRawDepthOfImage32(int width, int height, int rowStep = 0) {
  return hipRawDepthOfCloud(width, height, 4, rowStep ? rowStep : 4 * width, 0);
}
// OpenNI's 16-bit image in millimetres (0 = no reading), rows of rowStep bytes (0: packed)
inline mh_raw_depth hipRawDepthOfImage16(int width, int height, int rowStep = 0) {
  mh_raw_depth r = hipRawDepthOfCloud(width, height, 2, rowStep ? rowStep : 2 * width, 0);
  r.format = MH_RAW_DEPTH_U16_MM;
  return r;
}

// depthmap := the IMAGE_TYPE_DEPTH_MAP image of the frame (:270-279, :306-333).  false: no device or a refused argument
// (HipSession::warn has said which); depthmap then holds its header and a zeroed buffer of the right size.
inline bool hipKinectDepthmap(Image& depthmap, const void* raw, const mh_raw_depth& desc, const Pt<4>& linearCalibration,
                              const Pt<4>& nonlinearCalibration, int width, int height) {
  depthmap.name = "Depthmap";
  depthmap.imageType = IMAGE_TYPE_DEPTH_MAP;
  depthmap.intrinsicLinearCalibration = linearCalibration;
  depthmap.intrinsicNonlinearCalibration = nonlinearCalibration;
  depthmap.cameraPose.translation.init(0.0, 0.0, 0.0);
  depthmap.cameraPose.rotation.init(0.0, 0.0, 0.0, 1.0);
  depthmap.width = width;
  depthmap.height = height;
  depthmap.data.assign(width > 0 && height > 0 ? (size_t)width * height * sizeof(Float) * 4 : 0, 0);
  mh_ctx* ctx = HipSession::get();
  if (!ctx || depthmap.data.empty()) return false;
  float K[4];
  for (int k = 0; k < 4; k++) K[k] = (float)linearCalibration[k];
  if (mh_depth_map_from_raw_host(ctx, raw, &desc, K, (float*)&depthmap.data[0], width, height) != MH_OK) {
    HipSession::warn("mh_depth_map_from_raw_host");
    return false;
  }
  return true;
}

}  // namespace MopedNS
