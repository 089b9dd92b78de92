// SENSOR_IMAGE_HIP -- the gray image of a frame from what the camera delivers, made on the device: the replacement for the
// first line of moped3d's image callback, cv_bridge::toCvCopy(iMsg, "mono8") (moped3d/moped3d.cpp:249), and for the copy
// loop behind it (:263-265).  It is no STEP: the node converts before the pipeline sees the frame.  In the node,
//
//     mh_raw_image fmt;
//     if( hipImageFormat( iMsg->encoding, iMsg->width, iMsg->height, iMsg->step, &fmt )
//         && hipSensorGray( 0, &iMsg->data[0], fmt, gsMoped->data ) ) {
//       gsMoped->width = fmt.width;  gsMoped->height = fmt.height;             // packed rows: no widthStep left
//     } else { ... the node's own cv_bridge line and copy loop (:249-265) ... }
//
// A Kinect delivers bgr8 on /camera/rgb/image_color and bayer_grbg8 on image_raw, the Prosilica cameras of moped2's launch
// files Bayer mosaics; mono8 goes the same way and only loses its row padding.  Any other encoding (16-bit, YUV,
// compressed) makes hipImageFormat return false and stays with cv_bridge.  The arithmetic restates OpenCV 2.x cvtColor
// for 8-bit data from knowledge of that code, without OpenCV at hand: it is UNPINNED (csrc/image_gray.hip has it; the
// definition the tests hold it to is tests/image_gray_ref.py).  moped2's node copies `width` bytes of every BGR8 row
// (moped2/moped.cpp:175-204): a defect this header does not reproduce -- a moped2 node calls these two functions the same
// way.  A host that keeps its frames on the device sets the format once (mh_frame_set_image_format) and hands the raw
// buffers to the frame calls instead; FRAME_RESIDENT_3D_HIP takes the gray image as before.
// Needs hip_session.hpp's HipSession only; clean under -std=gnu++98.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "hip_session.hpp"

namespace MopedNS {

// ROS's sensor_msgs/image_encodings.h names -> MH_IMAGE_*; -1: not one this header converts
inline int hipImageEncoding(const std::string& encoding) {
  static const char* const names[] = {"mono8", "bgr8", "rgb8", "bgra8", "rgba8", "bayer_rggb8", "bayer_bggr8",
                                      "bayer_gbrg8", "bayer_grbg8"};
  for (int i = 0; i < 9; i++)
    if (encoding == names[i]) return MH_IMAGE_GRAY8 + i;
  return -1;
}

// The description of a sensor_msgs/Image: encoding, width, height, step (bytes of a row; 0: packed).  false: an encoding
// the device does not convert -- the node keeps its cv_bridge line for it.
inline bool hipImageFormat(const std::string& encoding, int width, int height, int step, mh_raw_image* fmt) {
  const int format = hipImageEncoding(encoding);
  if (format < 0 || !fmt) return false;
  const int bpp = format == MH_IMAGE_BGR8 || format == MH_IMAGE_RGB8 ? 3 : format == MH_IMAGE_BGRA8 || format == MH_IMAGE_RGBA8 ? 4 : 1;
  fmt->format = format;
  fmt->width = width;
  fmt->height = height;
  fmt->row_stride = step ? step : width * bpp;
  fmt->offset = 0;
  return true;
}

// out := the packed [height][width] gray image of the camera's buffer (:249-265).  session 0 = the process's HipSession.
// false: no device, or a refused description (the log says which); out is then empty.
inline bool hipSensorGray(mh_ctx* session, const void* data, const mh_raw_image& fmt, std::vector<unsigned char>& out) {
  out.clear();
  mh_ctx* ctx = session ? session : HipSession::get();
  if (!ctx || fmt.width <= 0 || fmt.height <= 0) return false;
  out.assign((size_t)fmt.width * fmt.height, 0);
  if (mh_image_gray_host(ctx, data, &fmt, &out[0]) != MH_OK) {
    std::clog << "[moped_hip] mh_image_gray_host: " << mh_last_error(ctx) << std::endl;   // (as HipSession::warn, of this context)
    out.clear();
    return false;
  }
  return true;
}

}  // namespace MopedNS
