// CPU sanitizer run (ASan + UBSan; no GPU, no HIP runtime) of the model set's row interface: mh_models_add_rows and
// mh_models_write_xml (the file samples/createModels/createModels.cpp:121-126 writes), then the file back through
// mh_models_add_xml and the set through mh_models_save / mh_models_load.  `make asan` builds and runs it.
//
//   planar_xml_asan <scratch directory>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "moped_hip.h"

extern "C" int mh_db_upload_raw(mh_ctx*, const float*, const int32_t*, const float*, int, int, int32_t, int) {
  return MH_ERR_ARG;   // never reached: nothing here uploads (models.cpp names it, the HIP library defines it)
}

#define CHECK(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                               \
    }                                                         \
  } while (0)

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string xml = dir + "/planar_xml_asan.moped.xml", db = dir + "/planar_xml_asan.mopeddb";
  mh_model_set* s = nullptr;
  CHECK(mh_models_create(&s, nullptr) == MH_OK);
  unsigned state = 12345u;
  std::vector<int> sizes = {0, 1, 7, 300, 2, 0, 65};
  int total_models = 0;
  for (size_t m = 0; m < sizes.size(); ++m) {
    const int n = sizes[m];
    std::vector<float> desc((size_t)n * MH_DESC_DIM), xyz((size_t)n * 3);
    for (float& v : desc) v = (float)((state = state * 1664525u + 1013904223u) >> 8) / 16777216.f;
    for (float& v : xyz) v = (float)((state = state * 1664525u + 1013904223u) >> 8) / 16777216.f - 0.5f;
    if (n > 0) {   // what %g has to get right
      desc[0] = 0.f;
      desc[1] = 1e-05f;
      desc[2] = 123456.7f;
      desc[3] = -0.f;
      desc[4] = 1e-42f;
      desc[5] = 3.4e38f;
      xyz[2] = 0.f;
    }
    const std::string name = "model " + std::to_string(m % 5);   // names 0 and 1 come twice: replace by name
    const int before = mh_models_count(s);
    bool known = false;
    for (int i = 0; i < before; ++i) known = known || name == mh_models_name(s, i);
    // (n = 0: the arrays' pointers are not read)
    CHECK(mh_models_add_rows(s, name.c_str(), n ? desc.data() : nullptr, n ? xyz.data() : nullptr, n) == MH_OK);
    CHECK(mh_models_count(s) == before + (known ? 0 : 1));
    total_models = mh_models_count(s);
  }
  // rows that are views of the set's own arrays, replacing the model they come from
  int64_t b = 0, n = 0;
  CHECK(mh_models_range(s, 3, &b, &n, nullptr) == MH_OK && n == 300);
  CHECK(mh_models_add_rows(s, mh_models_name(s, 3), mh_models_desc(s) + (b + 100) * MH_DESC_DIM, mh_models_xyz(s) + (b + 100) * 3,
                           150) == MH_OK);
  CHECK(mh_models_add_rows(s, "bad", nullptr, nullptr, -1) == MH_ERR_ARG);
  CHECK(mh_models_add_rows(s, "bad", nullptr, nullptr, 4) == MH_ERR_ARG);
  CHECK(mh_models_add_rows(s, nullptr, nullptr, nullptr, 0) == MH_ERR_ARG);
  CHECK(mh_models_count(s) == total_models);
  CHECK(mh_models_write_xml(s, total_models, xml.c_str()) == MH_ERR_ARG);
  CHECK(mh_models_write_xml(s, -1, xml.c_str()) == MH_ERR_ARG);
  // every model out and back in: the same name, the same number of rows, values equal to 6 digits
  for (int i = 0; i < total_models; ++i) {
    CHECK(mh_models_write_xml(s, i, xml.c_str()) == MH_OK);
    mh_model_set* r = nullptr;
    CHECK(mh_models_create(&r, nullptr) == MH_OK);
    CHECK(mh_models_add_xml(r, xml.c_str()) == MH_OK);
    int64_t rb = 0, rn = 0;
    CHECK(mh_models_range(s, i, &b, &n, nullptr) == MH_OK && mh_models_range(r, 0, &rb, &rn, nullptr) == MH_OK);
    CHECK(rn == n && std::strcmp(mh_models_name(r, 0), mh_models_name(s, i)) == 0);
    for (int64_t k = 0; k < n * MH_DESC_DIM; ++k) {
      const float want = mh_models_desc(s)[b * MH_DESC_DIM + k], got = mh_models_desc(r)[k];
      CHECK(std::fabs(got - want) <= 1e-5f * std::fabs(want));
    }
    mh_models_destroy(r);
  }
  CHECK(mh_models_save(s, db.c_str()) == MH_OK);
  mh_model_set* l = nullptr;
  CHECK(mh_models_load(&l, db.c_str()) == MH_OK);
  CHECK(mh_models_count(l) == total_models && mh_models_rows(l) == mh_models_rows(s));
  CHECK(std::memcmp(mh_models_desc(l), mh_models_desc(s), (size_t)mh_models_rows(s) * MH_DESC_DIM * sizeof(float)) == 0);
  CHECK(mh_models_add_rows(l, "x", nullptr, nullptr, 0) == MH_ERR_ARG);   // a mapped set is read-only
  CHECK(mh_models_write_xml(l, 3, xml.c_str()) == MH_OK);                 // ... but prints
  mh_models_destroy(l);
  mh_models_destroy(s);
  std::remove(xml.c_str());
  std::remove(db.c_str());
  std::printf("planar_xml_asan: %d models written, read back, saved and loaded\n", total_models);
  return 0;
}
