// object_hulls_hip.hpp against the reference's REAL include/moped.hpp (`make check_ref_hulls`: moped2 and moped3d): Pt,
// Pose, Model, Image and Object are then the reference's own types, util.hpp's part comes from the mirror (see check_ref.cpp).
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <moped.hpp>
#include "moped_util_mirror.hpp"
#include "object_hulls_hip.hpp"
int main() { return 0; }
