// Syntax check of the moped3d DEPTH_VERIFY step header at the reference's language level.
#include <tr1/memory>
namespace std { using tr1::shared_ptr; }
#define MOPED_AMD_WITH_DEPTH
#include "moped_types.hpp"
#include "DEPTH_VERIFY_HIP.hpp"
int main() { return 0; }
