// hull.hip: getObjectHull for a list of objects, one workgroup each (see there).
#pragma once
#include "steps.h"

namespace mh {

// what the walk over one object needs, whoever names the object
struct HullCore {
  const float* xyz;             // the store's rows [N][3]
  const int32_t* model_begin;   // device [n_models + 1]: model m's rows are [model_begin[m], model_begin[m + 1])
  int n_models;
  DevCam cam;
  int max_vertices;             // >= 1
  int form;                     // 0: the octagon prefilter; 1: sort and chain everything (mh_hull_debug_form)
  float2* scratch;              // global scratch for objects with more than MH_HULL_LDS_POINTS survivors, or nullptr
  size_t scratch_stride;        // ... points per object (list) or per workgroup (frames): hull_scratch_points of the largest model
};

// mh_object_hulls: a list of objects
struct HullArgs {
  HullCore core;
  const int32_t* obj_model;     // device [n_obj]
  const float* obj_pose;        // device [n_obj][7]
  const int32_t* n_obj_dev;     // device word with the object count (clamped to n_obj), or nullptr: n_obj
  int n_obj;                    // the grid
  float* hull_xy;               // device [n_obj][max_vertices][2]: the first min(n_vertices, max_vertices) vertices
  int32_t* n_vertices;          // device [n_obj]: the true count (-1: the scratch was too small, nothing written)
  int32_t* n_behind;            // device [n_obj]: rows with z < 0.001, left out of the hull
  float* bbox_uv;               // device [n_obj][8][2]
};

// Frames: the objects of n_frames result slots ({int32 n; int32 pad[3]; mh_object[max_objects]}, frame.h) from first_slot
// on.  Object o of slot s gets record o of the slot's part of the hull block: hull_record_words(max_vertices) words --
// n_vertices, n_behind, corners [8][2], vertices [max_vertices][2].
constexpr int HULL_FRAME_GRID = 16;   // workgroups per frame (a frame has 2 - 10 objects; more are walked in turns)
__host__ __device__ constexpr size_t hull_record_words(int max_vertices) { return 18 + 2 * (size_t)max_vertices; }
struct HullFrameArgs {
  HullCore core;                // (cam: the frame's camera when cams == nullptr)
  const DevCam* cams;           // device table of the frame's cameras, or nullptr
  int image;                    // ... and the camera whose hulls are wanted
  const unsigned char* result;
  size_t result_bytes;
  int max_objects;
  int first_slot;
  unsigned char* block;         // the hull block: slot s at block + s * slot_bytes
  size_t slot_bytes;
};

// points of global scratch an object of a model with `rows` rows may need (0: the LDS path always suffices)
size_t hull_scratch_points(int rows);
void launch_object_hulls(const HullArgs& a, hipStream_t s);
void launch_frame_hulls(const HullFrameArgs& a, int n_frames, hipStream_t s);

}  // namespace mh
