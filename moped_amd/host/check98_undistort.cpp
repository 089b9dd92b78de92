// Syntax check of the UNDISTORTED_IMAGE step header at the reference's language level (built twice by the Makefile:
// plain, and with -DMOPED_AMD_WITH_DEPTH for moped3d's Image).
#include <tr1/memory>
namespace std { using tr1::shared_ptr; }
#include "moped_types.hpp"
#include "UTIL_UNDISTORT_HIP.hpp"
int main() { return 0; }
