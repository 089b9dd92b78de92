// createPlanarModelsFromImages_HIP compiled against the reference's REAL include/moped.hpp (`make check_ref_planar`), at
// the reference's language level: SP_Image, Float, toString and sXML are then the reference's own, and the function has
// the signature of Moped::createPlanarModelsFromImages (include/moped.hpp:385) with the session in front.  Only
// src/util.hpp's part comes from the mirror (util.hpp needs OpenCV).  Skipped where the reference is absent.
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <moped.hpp>
namespace std { using tr1::shared_ptr; }
#include "moped_util_mirror.hpp"
#include "planar_models_hip.hpp"

// the reference's member, and ours with the session in front
typedef std::vector<std::tr1::shared_ptr<sXML> > (Moped::*reference_call)(std::vector<MopedNS::SP_Image>&, float);
typedef std::vector<std::tr1::shared_ptr<sXML> > (*hip_call)(mh_ctx*, std::vector<MopedNS::SP_Image>&, MopedNS::Float, int, int,
                                                             const std::string&);

// (unevaluated: libmoped itself is not linked)
char (&takes_reference_call(reference_call))[1];
typedef char reference_signature_is_as_assumed[sizeof(takes_reference_call(&Moped::createPlanarModelsFromImages))];

int main() {
  hip_call f = &MopedNS::createPlanarModelsFromImages_HIP;
  // no session: an empty result, nothing touched; and the tree prints through the reference's sXML::print
  std::vector<MopedNS::SP_Image> images(1, MopedNS::SP_Image(new MopedNS::Image));
  images[0]->width = images[0]->height = 0;
  if (!f(0, images, 1.f, 1, 8192, "SIFT").empty()) return 1;
  sXML x;
  x.name = "Model";
  x["name"] = "m";
  x.children.resize(1);
  x.children[0].name = "Points";
  std::ostringstream out;
  x.print(out);
  return out.str() == "<Model name=\"m\">\n\t<Points/>\n</Model>\n" ? 0 : 2;
}
