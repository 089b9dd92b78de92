// Records what the reference's own getConvexHull (include/moped.hpp:293-327) returns for the clouds of a case file.
// Test infrastructure of tests/tools/make_hull_golden.py: built against the reference header where it lies
// (-I <reference>/moped2/libmoped/include), run once when the golden is made, never needed by a test.
//
//   in : int32 n_cases, int32 off[n_cases + 1], float32 pts[off[n_cases]][2]
//   out: int32 n_cases, int32 hoff[n_cases + 1], float32 hull[hoff[n_cases]][2]
#include <moped.hpp>

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int n_cases = 0;
  if (fread(&n_cases, 4, 1, in) != 1) return 4;
  std::vector<int> off(n_cases + 1);
  if (fread(&off[0], 4, off.size(), in) != off.size()) return 4;
  std::vector<float> pts(2 * (size_t)off[n_cases] + 2);
  if (off[n_cases] > 0 && fread(&pts[0], 8, off[n_cases], in) != (size_t)off[n_cases]) return 4;
  fclose(in);

  std::vector<int> hoff(1, 0);
  std::vector<float> hull;
  for (int c = 0; c < n_cases; ++c) {
    std::vector<MopedNS::Pt<2> > cloud;
    for (int i = off[c]; i < off[c + 1]; ++i) {
      MopedNS::Pt<2> p;
      p.init(pts[2 * i], pts[2 * i + 1]);
      cloud.push_back(p);
    }
    if (!cloud.empty()) {   // (an empty cloud is undefined behaviour in the reference: *points.begin())
      std::list<MopedNS::Pt<2> > h = MopedNS::getConvexHull(cloud);
      for (std::list<MopedNS::Pt<2> >::const_iterator it = h.begin(); it != h.end(); ++it) {
        hull.push_back((*it)[0]);
        hull.push_back((*it)[1]);
      }
    }
    hoff.push_back((int)(hull.size() / 2));
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 5;
  fwrite(&n_cases, 4, 1, out);
  fwrite(&hoff[0], 4, hoff.size(), out);
  if (!hull.empty()) fwrite(&hull[0], 4, hull.size(), out);
  fclose(out);
  return 0;
}
