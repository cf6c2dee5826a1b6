// Host-only helpers of the set-up objects (gqMeshSet, gqBvh, gqPointGrid, gqHand): the owner of their memory and the
// Morton ordering of a mesh's faces.  Nothing here runs per step.
#pragma once
#include "common.h"

#include "cluster_bound.h"  // gq_box_of, gq_morton_order: the Morton ordering of a mesh's faces

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

// sdf.hip: rec[i] = record of face perm[i] of the device triangles fv for i < F, a far-away padding record for F <= i < Fp
struct GqFace;
int gq_face_records_(const float* fv, const int32_t* perm, int64_t F, int64_t Fp, GqFace* rec, hipStream_t st);
