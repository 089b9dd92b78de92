// DEPTH_VERIFY_HIP.hpp against moped3d's REAL include/moped.hpp (`make check_ref_depth_verify`): Pt, Image, Object and
// FrameData's members are then the reference's own types, util.hpp's part comes from the mirror (see check_ref.cpp).
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <moped.hpp>
#define MOPED_AMD_WITH_DEPTH 1
#include "moped_util_mirror.hpp"
#include "DEPTH_VERIFY_HIP.hpp"
int main() { return 0; }
