// depth_verify.hip: DEPTH_VERIFY_CPU::process for a list of objects, one workgroup each (see there).
#pragma once
#include "steps.h"

namespace mh {

constexpr int DV_THREADS = 256;
constexpr int DV_CHUNK = MH_DEPTH_VERIFY_CHUNK;   // terms the producing wavefronts hand the chaining one per round
constexpr int DV_GRID = 128;                      // grid stride over the objects
static_assert(DV_CHUNK == DV_THREADS - 64, "one term per producing thread and round");

// what the walk over one object needs, whoever names the object
struct DepthVerifyArgs {
  const float* xyz;             // the store's rows [N][3]: the keypoints of model m are rows [model_begin[m], model_begin[m + 1])
  const int32_t* model_begin;   // device [n_models + 1]
  const float4* img;            // the depth map [h][w] (x, y, z, norm): z is word 2 (Image::getDepth)
  const float* fill;            // its distance map [h][w], or nullptr: no distance test
  int w, h;
  DevCam cam;                   // the image the matches were found in (project(), :129)
  DevCam dcam;                  // the depth map's K and pose (:105, :162)
  float feature_distance, max_multiplier, max_distance, depth_fraction;   // the constructor's arguments (:64)
};

// mh_depth_verify: a list of objects against one match list
struct DepthVerifyListArgs {
  DepthVerifyArgs core;
  const mh_corr* corr;          // device: matches[m] = corr[model_off[m] .. model_off[m + 1])
  const int32_t* model_off;     // device [n_models + 1]
  const int32_t* obj_model;     // device [n_obj]
  const float* obj_pose;        // device [n_obj][7]
  int n_obj;
  mh_verify_record* rec;        // device [n_obj]
};

// Frames (mh_frame_set_depth_verify): the objects of n_frames result slots ({int32 n; int32 pad[3]; mh_object[max_objects]},
// frame.h) from first_slot on, frame f against its own arena's match lists and its own map.  Workgroup (x, f) scores the
// objects x, x + gridDim.x, ... of slot first_slot + f into the slot's part of the record block -- {int32 n_before; int32
// pad[3]; mh_verify_record[max_objects]}, in the order before the erase -- and the frame's last workgroup to finish removes
// the erased objects from the result slot, stably, and lowers its count.
constexpr int DV_FRAME_GRID = 16;   // workgroups per frame (a frame has 2 - 10 objects; more are walked in turns)
struct DepthVerifyFrameArgs {
  DepthVerifyArgs core;         // (img / fill: the frame's map when maps_on == 0)
  DepthMaps maps;               // maps_on: frame f's map
  int maps_on;
  const mh_corr* corr;          // frame 0's arena: m_corr and model_off; frame f's lie arena_bytes * f further
  const int32_t* model_off;
  size_t arena_bytes;
  unsigned char* result;        // the result slots
  size_t result_bytes;
  int max_objects;
  int first_slot;
  unsigned char* block;         // the record block: slot s at block + s * slot_bytes
  size_t slot_bytes;
  unsigned int* tickets;        // [MH_MAX_BATCH], zero before the first launch
};
void launch_frame_depth_verify(const DepthVerifyFrameArgs& a, int n_frames, hipStream_t s);

// form 0: a workgroup per object, three wavefronts produce the terms, one chains them; 1: a wavefront per object
void launch_depth_verify(const DepthVerifyListArgs& a, int form, hipStream_t s);

}  // namespace mh
