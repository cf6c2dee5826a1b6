// What a header of graspqp_amd/csrc asks of its includer when a HOST compiler builds it (common.h provides it in the library): the
// qualifiers as no-ops, GQ_INF_F, gq3 / gq_mk, min, and the structs of the public header.  Every tests/*_host.cpp starts here;
// GQ_SCENE_HOST_BUILD keeps the csrc headers from including common.h (and with it the HIP runtime).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>
using std::min;
#define GQ_SCENE_HOST_BUILD
#define __device__
#define __forceinline__ inline
#define GQ_INF_F __builtin_inff()
#include "../include/graspqp_hip.h"
struct gq3 {
  float x, y, z;
};
static inline gq3 gq_mk(float x, float y, float z) { return gq3{x, y, z}; }
