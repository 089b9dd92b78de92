// Syntax check of the moped3d depth FILTER step header at the reference's language level.
#include <tr1/memory>
namespace std { using tr1::shared_ptr; }
#define MOPED_AMD_WITH_DEPTH
#include "moped_types.hpp"
#include "FILTER_PROJECTION_HIP.hpp"
#include "FILTER_PROJECTION_DEPTH_HIP.hpp"
int main() { return 0; }
