// UTIL_UNDISTORT_HIP.hpp against the reference's REAL include/moped.hpp (`make check_ref`): moped2's, and moped3d's
// with -DMOPED_AMD_WITH_DEPTH (Image::imageType); util.hpp's part from the mirror (see check_ref.cpp).
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <moped.hpp>
#include "moped_util_mirror.hpp"
#include "UTIL_UNDISTORT_HIP.hpp"

int main() {
  MopedNS::MopedPipeline pipeline;
  pipeline.addAlg("UNDISTORTED_IMAGE", new MopedNS::UTIL_UNDISTORT_HIP);
  return 0;
}
