// Host-only helpers of the set-up objects (gqMeshSet, gqBvh, gqPointGrid, gqHand): the owner of their memory and the
// Morton ordering of a mesh's faces.  Nothing here runs per step.
#pragma once
#include "common.h"

#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <utility>
#include <vector>

// allocations currently held by all owners of the process (gq_setup_live_allocations)
inline std::atomic<int64_t> gq_setup_live_{0};

// Owns every device and host allocation of one object, or the scratch buffers of one create call, and frees them when it
// goes out of scope -- on every return path.  The first failure sticks in `rc` (message in gq_last_error) and turns the
// later calls into no-ops that return null, so a create function checks `rc` once, before its first launch.
class GqOwner {
 public:
  int rc = GQ_OK;
  GqOwner() = default;
  GqOwner(const GqOwner&) = delete;
  GqOwner& operator=(const GqOwner&) = delete;
  ~GqOwner() {
    for (void* p : dev_) (void)hipFree(p);
    for (void* p : host_) free(p);
    gq_setup_live_ -= (int64_t)(dev_.size() + host_.size());
  }
  template <typename T>
  T* alloc(size_t n) {  // device; zero elements give a null pointer
    void* p = nullptr;
    if (n == 0 || rc || (rc = check(hipMalloc(&p, n * sizeof(T)), "hipMalloc"))) return nullptr;
    return (T*)keep(dev_, p);
  }
  template <typename T>
  T* upload(const T* src, size_t n) {
    T* p = alloc<T>(n);
    if (p) rc = check(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    return rc ? nullptr : p;
  }
  template <typename T>
  T* host_copy(const T* src, size_t n) {
    if (n == 0 || rc) return nullptr;
    void* p = malloc(n * sizeof(T));
    if (!p) {
      rc = check(hipErrorOutOfMemory, "malloc");
      return nullptr;
    }
    memcpy(p, src, n * sizeof(T));
    return (T*)keep(host_, p);
  }
  void adopt(GqOwner& o) {  // take over what `o` holds (a part built aside until it is complete)
    dev_.insert(dev_.end(), o.dev_.begin(), o.dev_.end());
    host_.insert(host_.end(), o.host_.begin(), o.host_.end());
    o.dev_.clear();
    o.host_.clear();
  }

 private:
  std::vector<void*> dev_, host_;
  static void* keep(std::vector<void*>& v, void* p) {
    v.push_back(p);
    ++gq_setup_live_;
    return p;
  }
  static int check(hipError_t e, const char* what) {
    if (e == hipSuccess) return GQ_OK;
    GQ_FAIL(GQ_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
  }
};

// ---- Morton order of a mesh's faces ------------------------------------------------------------------------------------
static inline uint32_t gq_spread10(uint32_t v) {
  v &= 0x3ff;
  v = (v | (v << 16)) & 0x030000ff;
  v = (v | (v << 8)) & 0x0300f00f;
  v = (v | (v << 4)) & 0x030c30c3;
  v = (v | (v << 2)) & 0x09249249;
  return v;
}

// box (lo.xyz, 0, hi.xyz, 0) of the faces perm[a..b)
static inline void gq_box_of(const float* fv, const int32_t* perm, int64_t a, int64_t b, float* out8) {
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int64_t i = a; i < b; ++i) {
    const float* v = fv + (int64_t)perm[i] * 9;
    for (int k = 0; k < 9; ++k) {
      const int c = k % 3;
      lo[c] = v[k] < lo[c] ? v[k] : lo[c];
      hi[c] = v[k] > hi[c] ? v[k] : hi[c];
    }
  }
  out8[0] = lo[0]; out8[1] = lo[1]; out8[2] = lo[2]; out8[3] = 0.0f;
  out8[4] = hi[0]; out8[5] = hi[1]; out8[6] = hi[2]; out8[7] = 0.0f;
}

// perm[begin..end) = the faces begin .. end-1 ordered along the 30-bit Morton curve of their centroids inside `box`
// (gq_box_of layout); faces with equal codes keep their index order
static inline void gq_morton_order(const float* fv, int32_t* perm, int64_t begin, int64_t end, const float* box) {
  std::vector<std::pair<uint32_t, int32_t>> keys;
  keys.reserve(end - begin);
  for (int64_t i = begin; i < end; ++i) {
    const float* v = fv + i * 9;
    uint32_t code = 0;
    for (int c = 0; c < 3; ++c) {
      const float ctr = (v[c] + v[3 + c] + v[6 + c]) * (1.0f / 3.0f);
      const float ext = box[4 + c] - box[c];
      float t = ext > 0.0f ? (ctr - box[c]) / ext : 0.0f;
      t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
      code |= gq_spread10((uint32_t)(t * 1023.0f)) << c;
    }
    keys.emplace_back(code, (int32_t)i);
  }
  std::stable_sort(keys.begin(), keys.end());
  for (int64_t i = begin; i < end; ++i) perm[i] = keys[i - begin].second;
}

// sdf.hip: rec[i] = record of face perm[i] of the device triangles fv for i < F, a far-away padding record for F <= i < Fp
struct GqFace;
int gq_face_records_(const float* fv, const int32_t* perm, int64_t F, int64_t Fp, GqFace* rec, hipStream_t st);
