// undistort_step_test -- the first two slots of the reference's pipeline, UNDISTORTED_IMAGE (UTIL_UNDISTORT_HIP) then
// SIFT (FEAT_SIFT_HIP), over frames of 8-bit PGM images, each image with its own calibration:
//
//   undistort_step_test img.pgm fx fy cx cy k1 k2 p1 p2 [img.pgm ...] [--frame img.pgm ...]
//
// "--frame" starts the next frame.  Per frame and image it prints the undistorted bytes (hex) and the keypoints the
// SIFT step appended for that image:
//   FRAME f / IMAGE i w h / BYTES <hex> / KEYPOINTS n / KP i col row checksum
// checksum = sum over k of descriptor[k] (k + 1) (as moped_hip_test --sift prints it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "moped_types.hpp"

#include "FEAT_SIFT_HIP.hpp"
#include "UTIL_UNDISTORT_HIP.hpp"

using namespace MopedNS;

static SP_Image read_pgm(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return SP_Image();
  int w = 0, h = 0, maxv = 0;
  SP_Image image(new Image);
  if (std::fscanf(f, "P5 %d %d %d", &w, &h, &maxv) != 3 || maxv != 255 || w <= 0 || h <= 0) {
    std::fclose(f);
    return SP_Image();
  }
  std::fgetc(f);
  image->width = w;
  image->height = h;
  image->name = path;
  image->data.resize((size_t)w * h);
  const bool ok = std::fread(&image->data[0], 1, image->data.size(), f) == image->data.size();
  std::fclose(f);
  return ok ? image : SP_Image();
}

int main(int argc, char** argv) {
  vector<vector<SP_Image> > frames(1);
  for (int a = 1; a < argc;) {
    if (std::string(argv[a]) == "--frame") {
      frames.push_back(vector<SP_Image>());
      ++a;
      continue;
    }
    if (a + 9 > argc) {
      std::fprintf(stderr, "usage: undistort_step_test img.pgm fx fy cx cy k1 k2 p1 p2 ... [--frame ...]\n");
      return 2;
    }
    SP_Image image = read_pgm(argv[a]);
    if (!image) {
      std::perror(argv[a]);
      return 2;
    }
    for (int k = 0; k < 4; ++k) {
      image->intrinsicLinearCalibration[k] = (Float)std::atof(argv[a + 1 + k]);
      image->intrinsicNonlinearCalibration[k] = (Float)std::atof(argv[a + 5 + k]);
    }
    frames.back().push_back(image);
    a += 9;
  }

  MopedPipeline pipeline;
  pipeline.addAlg("UNDISTORTED_IMAGE", new UTIL_UNDISTORT_HIP);
  pipeline.addAlg("SIFT", new FEAT_SIFT_HIP("-1"));
  list<MopedAlg*> algs = pipeline.getAlgs(true);
  if (algs.size() != 2) return 3;   // no device: the steps are not capable

  for (size_t f = 0; f < frames.size(); ++f) {
    list<SP_Object> objects;
    FrameData frameData;
    frameData.objects = &objects;
    frameData.images = frames[f];
    for (list<MopedAlg*>::iterator it = algs.begin(); it != algs.end(); ++it) (*it)->process(frameData);
    std::printf("FRAME %zu\n", f);
    const vector<FrameData::DetectedFeature>& feats = frameData.detectedFeatures["SIFT"];
    for (size_t i = 0; i < frameData.images.size(); ++i) {
      const Image& image = *frameData.images[i];
      std::printf("IMAGE %zu %d %d\nBYTES ", i, image.width, image.height);
      for (size_t p = 0; p < image.data.size(); ++p) std::printf("%02x", image.data[p]);
      size_t n = 0;
      for (size_t k = 0; k < feats.size(); ++k) n += feats[k].imageIdx == (int)i;
      std::printf("\nKEYPOINTS %zu\n", n);
      for (size_t k = 0; k < feats.size(); ++k) {
        if (feats[k].imageIdx != (int)i) continue;
        double sum = 0;
        for (int d = 0; d < 128; ++d) sum += feats[k].descriptor[d] * (d + 1);
        std::printf("KP %d %.9g %.9g %.17g\n", feats[k].imageIdx, feats[k].coord2D[0], feats[k].coord2D[1], sum);
      }
    }
  }
  return 0;
}
