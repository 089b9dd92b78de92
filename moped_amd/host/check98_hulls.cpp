// Syntax check of object_hulls_hip.hpp at the reference's language level, against the mirror of its types.
#include <tr1/memory>
namespace std { using tr1::shared_ptr; }
#include "moped_types.hpp"
#include "object_hulls_hip.hpp"
int main() { return 0; }
