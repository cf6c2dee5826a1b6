// Objects as oriented point clouds: the contact query against N oriented discs (surfels) instead of a triangle mesh.
//
// A cloud is N points p_i with unit outward normals n_i and one radius rho > 0.  For a query x (include/graspqp_hip.h):
//   j = argmin_i |x - p_i|^2 (ties to the smallest index);  v = x - p_j, h = v . n_j, lat = v - h n_j, l = |lat|;
//   closest = p_j + lat min(1, rho / l);  dist_sq = |x - closest|^2;  sign = h >= 0 ? +1 : -1;
//   normal = sign n_j on the disc (l <= rho), (x - closest)/|x - closest| beyond its rim.
// The outputs have the layout and meaning of gq_sdf_forward_meshset, so everything downstream reads them unchanged.
//
// Set-up (gq_cloudset_create, host): per cloud a uniform grid with ONE cell width h on all three axes (a few points per
// occupied cell), the points sorted by cell with x running fastest, and a cell-start table.  A row of cells along x at fixed
// (y,z) is therefore one contiguous range of the sorted points.  An axis along which the cloud has no extent gets one cell of
// width h (no zero-width cells); a cloud without any extent gets h = rho.
//
// Query (one wavefront per query; the stepper's call has 3 072 of them, too few for one query per lane): the query's cell is
// clamped into the grid.  Every lane keeps its best candidate as the key (bits of d^2) << 32 | original index, whose unsigned
// minimum over the wavefront is the brute-force winner with the index tie rule.
//   Stage 1 scans the 3 x 3 x 3 cells around the query's cell as 9 rows with 7 lanes per row.  Every point outside that cube
// lies at least two cells away along some axis a, so with e_a = the query's distance to the grid box along a (0 inside)
//   d^2 >= sum_b e_b^2 + h^2 + 2 h min_a e_a  =: bound
// and the search ends there only when bound > best d^2 (strictly: an equal distance with a smaller index could still win) or
// the cube covers the grid.  h enters the bound shrunk by 1e-4, which covers the fp32 rounding of the cell indices (<= 128
// cells per axis).  This is the case of a contact at the surface.
//   Stage 2, otherwise, is a ball query with the radius sqrt(best) -- of the cube's best, or, if the cube was empty, of up
// to 256 points spread over the sorted cloud.  The winner is within that radius by definition, so it lies in a row of cells
// whose (y,z) rectangle is within the radius of the query's (y,z), inside the cells that the ball's slice at that rectangle
// reaches along x.  Lanes take one row each (64 rows per pass), scan the slice's cells, and the wavefront's minimum after
// every pass shrinks the radius for the next.  Every comparison is inclusive and every rectangle and slice is widened by a
// margin for rounding, so a point at exactly the best distance is still seen: the result is the brute-force winner, and the
// loop runs over a fixed number of rows (at most the grid's n_y n_z), so it terminates.
//
// No LDS, no scratch, no atomics: results are bitwise reproducible run to run.
#include "common.h"
#include "setup.h"

#include <math.h>

#include <memory>

#define GQ_CLOUD_MAX_POINTS (1 << 20)
#define GQ_CLOUD_SHRINK 0.9999f  // on h in the bound of stage 1: rounding of the cell indices

struct GqCloud {  // 64 bytes
  float lo[3], inv_h;
  float hi[3], h;
  int32_t n[3];      // cells per axis
  float rho;
  int32_t cell_off;  // of this cloud's table in cell_start
  int32_t pt_off, pt_end;  // its range of the sorted points
  int32_t pad;
};

struct gqCloudSet {
  GqOwner mem;
  int n_obj = 0;
  int32_t* off_host = nullptr;  // (n_obj+1)
  float* rho_host = nullptr;    // (n_obj)
  const GqCloud* clouds = nullptr;
  const float4* pts = nullptr;  // sorted by cell: x y z, original index within the cloud (int bits)
  const float4* nrm = nullptr;  // same order: unit normal
  const int32_t* cell_start = nullptr;  // per cloud n_cells + 1 positions into pts
};

struct GqCloudArgs {
  const GqCloud* clouds;
  const float4* pts;
  const float4* nrm;
  const int32_t* cell_start;
  const float* points;
  int64_t N, qpo;
  float* dist_sq;
  int32_t* sign;
  float* normal;  // or null
  float* closest;
};

__device__ __forceinline__ float gq_uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ void gq_cloud_rank(const float4 P, int p, float x, float y, float z, unsigned long long& key, int& pos) {
  const float dx = x - P.x, dy = y - P.y, dz = z - P.z;
  const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
  // d2 >= 0: its bit pattern orders like its value; NaN / inf never beat the initial key
  const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(P.w);
  if (d2 < GQ_INF_F && k < key) key = k, pos = p;
}

// the points p0, p0 + step, ... below p1: four records in flight per round (an index past the end repeats the last point,
// which changes nothing)
__device__ __forceinline__ void gq_cloud_scan(const float4* __restrict__ pts, int p0, int p1, int step, float x, float y, float z,
                                              unsigned long long& key, int& pos) {
  for (int p = p0; p < p1; p += 4 * step) {
    const int i1 = min(p + step, p1 - 1), i2 = min(p + 2 * step, p1 - 1), i3 = min(p + 3 * step, p1 - 1);
    const float4 A = pts[p], B = pts[i1], C = pts[i2], D = pts[i3];
    gq_cloud_rank(A, p, x, y, z, key, pos);
    gq_cloud_rank(B, i1, x, y, z, key, pos);
    gq_cloud_rank(C, i2, x, y, z, key, pos);
    gq_cloud_rank(D, i3, x, y, z, key, pos);
  }
}

// lower bound of d^2 (as the kernel computes it) of every point outside the scanned cube (rh = one cell, shrunk); the factor covers
// the rounding of the bound itself and of a candidate's d^2 (a few fp32 ulps each)
__device__ __forceinline__ float gq_cloud_bound(float rh, float emin, float dbox2) {
  return fmaf(2.0f * rh, emin, fmaf(rh, rh, dbox2)) * (1.0f - 1e-6f);
}

// unsigned minimum of the keys over the wavefront; `pos` of the lane that holds it (keys are distinct: the index is in them)
__device__ __forceinline__ void gq_cloud_wave_min(unsigned long long& key, int& pos) {
  unsigned long long m = key;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)(m & 0xffffffffull), o, GQ_WAVE);
    const unsigned hi = __shfl_xor((unsigned)(m >> 32), o, GQ_WAVE);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    m = other < m ? other : m;
  }
  const unsigned long long owners = __ballot(key == m && pos >= 0);
  const int src = owners ? (int)__builtin_ctzll(owners) : 0;
  pos = owners ? __builtin_amdgcn_readlane(pos, src) : -1;
  key = m;
}

__global__ __launch_bounds__(256) void gq_cloud_wave_kernel(const GqCloudArgs a) {
  const int lane = gq_lane();
  const int64_t q = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / GQ_WAVE));
  if (q >= a.N) return;  // wave-uniform
  const GqCloud c = a.clouds[q / a.qpo];
  const float x = gq_uniform_f(a.points[q * 3]), y = gq_uniform_f(a.points[q * 3 + 1]), z = gq_uniform_f(a.points[q * 3 + 2]);
  const int nx = c.n[0], ny = c.n[1], nz = c.n[2];
  // clamped cell of the query (clamped as a float: a NaN coordinate gives cell 0) and its distance to the grid box per axis
  const int cx = (int)fminf(fmaxf(floorf((x - c.lo[0]) * c.inv_h), 0.0f), (float)(nx - 1));
  const int cy = (int)fminf(fmaxf(floorf((y - c.lo[1]) * c.inv_h), 0.0f), (float)(ny - 1));
  const int cz = (int)fminf(fmaxf(floorf((z - c.lo[2]) * c.inv_h), 0.0f), (float)(nz - 1));
  const float ex = fmaxf(fmaxf(c.lo[0] - x, x - c.hi[0]), 0.0f), ey = fmaxf(fmaxf(c.lo[1] - y, y - c.hi[1]), 0.0f),
              ez = fmaxf(fmaxf(c.lo[2] - z, z - c.hi[2]), 0.0f);
  const float dbox2 = fmaf(ex, ex, fmaf(ey, ey, ez * ez)), emin = fminf(ex, fminf(ey, ez));
  const int rcover = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));  // cube radius that holds the grid
  const float hs = c.h * GQ_CLOUD_SHRINK;
  const int32_t* __restrict__ cs = a.cell_start + c.cell_off;
  unsigned long long key = ~0ull;
  int pos = -1;
  {  // stage 1: the 3 x 3 x 3 cells around the query's cell as 9 rows of up to three cells, 7 lanes per row
    const int it = lane / 7, s = lane % 7;
    const int yy = cy + it / 3 - 1, zz = cz + it % 3 - 1;
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, nx - 1);
    if (lane < 63 && yy >= 0 && yy < ny && zz >= 0 && zz < nz) {
      const int row = (zz * ny + yy) * nx;
      const int p1 = cs[row + x1 + 1];
      gq_cloud_scan(a.pts, cs[row + x0] + s, p1, 7, x, y, z, key, pos);
    }
  }
  gq_cloud_wave_min(key, pos);
  float best = __uint_as_float((unsigned)(key >> 32));  // NaN pattern while nothing was found: compares false
  if (!(rcover <= 1 || gq_cloud_bound(hs, emin, dbox2) > best)) {
    if (pos < 0) {  // nothing within the cube: seed the radius with up to 256 points spread over the sorted cloud
      const int N = c.pt_end - c.pt_off, n_s = min(N, 4 * GQ_WAVE), stride = N / n_s;
      gq_cloud_scan(a.pts, c.pt_off + lane * stride, c.pt_off + n_s * stride, GQ_WAVE * stride, x, y, z, key, pos);
      gq_cloud_wave_min(key, pos);
      best = __uint_as_float((unsigned)(key >> 32));
    }
    if (pos >= 0) {
      // stage 2, ball query: every point within sqrt(best) of the query lies in a row (y,z) of cells whose rectangle is within
      // that distance of the query's (y,z), and there in the cells the ball's slice reaches along x.  m widens every
      // rectangle and slice: rounding of the cell indices at set-up and of coordinates of the query's magnitude.
      const float m = fmaf(4e-7f, fabsf(x) + fabsf(y) + fabsf(z) + sqrtf(best), 1e-3f * c.h);
      const float LIM = 1e6f;  // cell coordinates of a far query are bounded so that the int arithmetic cannot overflow
      const int qy = (int)fminf(fmaxf(floorf((y - c.lo[1]) * c.inv_h), -LIM), LIM);
      const int qz = (int)fminf(fmaxf(floorf((z - c.lo[2]) * c.inv_h), -LIM), LIM);
      const int k = (int)fminf((sqrtf(best) + m) * c.inv_h, LIM) + 2;
      const int y0 = max(qy - k, 0), y1 = min(qy + k, ny - 1), z0 = max(qz - k, 0), z1 = min(qz + k, nz - 1);
      const int wy = y1 - y0 + 1, wz = z1 - z0 + 1;
      const int n_rows = wy > 0 && wz > 0 ? wy * wz : 0;
      for (int base = 0; base < n_rows; base += GQ_WAVE) {  // lanes over rows; the radius shrinks from pass to pass
        const int it = base + lane;
        if (it < n_rows) {
          const int yy = y0 + it % wy, zz = z0 + it / wy;
          float yb = c.lo[1] + (float)(yy + 1) * c.h, zb = c.lo[2] + (float)(zz + 1) * c.h;
          if (yy == ny - 1) yb = fmaxf(yb, c.hi[1]);  // the last cell of an axis holds everything up to the box
          if (zz == nz - 1) zb = fmaxf(zb, c.hi[2]);
          const float dy = fmaxf(fmaxf(c.lo[1] + (float)yy * c.h - m - y, y - yb - m), 0.0f);
          const float dz = fmaxf(fmaxf(c.lo[2] + (float)zz * c.h - m - z, z - zb - m), 0.0f);
          const float rr = __uint_as_float((unsigned)(key >> 32)) * (1.0f + 4e-6f), dyz2 = fmaf(dy, dy, dz * dz);
          if (dyz2 <= rr) {
            const float wx = sqrtf(rr - dyz2) + m;
            int xa = (int)fminf(fmaxf(floorf((x - wx - c.lo[0]) * c.inv_h), -1.0f), (float)nx) - 1;
            int xb = (int)fminf(fmaxf(floorf((x + wx - c.lo[0]) * c.inv_h), -1.0f), (float)nx) + 1;
            xa = max(xa, 0), xb = min(xb, nx - 1);
            if (xa <= xb) {
              const int row = (zz * ny + yy) * nx;
              const int p1 = cs[row + xb + 1];
              gq_cloud_scan(a.pts, cs[row + xa], p1, 1, x, y, z, key, pos);
            }
          }
        }
        gq_cloud_wave_min(key, pos);
      }
    }
  }
  if (lane != 0) return;
  float d2o, clx, cly, clz, nox, noy, noz;
  int sg = 1;
  if (pos < 0) {  // a non-finite query: no candidate
    d2o = clx = cly = clz = nox = noy = noz = __builtin_nanf("");
  } else {
#pragma clang fp contract(off)
    const float4 P = a.pts[pos], Nj = a.nrm[pos];
    const float vx = x - P.x, vy = y - P.y, vz = z - P.z;
    const float h = vx * Nj.x + vy * Nj.y + vz * Nj.z;
    const float lx = vx - h * Nj.x, ly = vy - h * Nj.y, lz = vz - h * Nj.z;
    const float l = sqrtf(lx * lx + ly * ly + lz * lz);
    const bool on_disc = l <= c.rho;
    const float sc = on_disc ? 1.0f : c.rho / l;
    clx = P.x + lx * sc, cly = P.y + ly * sc, clz = P.z + lz * sc;
    const float rx = x - clx, ry = y - cly, rz = z - clz;
    d2o = rx * rx + ry * ry + rz * rz;
    sg = h >= 0.0f ? 1 : -1;
    if (on_disc) {
      nox = (float)sg * Nj.x, noy = (float)sg * Nj.y, noz = (float)sg * Nj.z;
    } else {
      const float inv = 1.0f / sqrtf(d2o);
      nox = rx * inv, noy = ry * inv, noz = rz * inv;
    }
  }
  a.dist_sq[q] = d2o;
  a.sign[q] = sg;
  a.closest[q * 3] = clx, a.closest[q * 3 + 1] = cly, a.closest[q * 3 + 2] = clz;
  if (a.normal) a.normal[q * 3] = nox, a.normal[q * 3 + 1] = noy, a.normal[q * 3 + 2] = noz;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static inline int gq_cloud_cell_(float v, float lo, float inv_h, int n) {
  const float t = floorf((v - lo) * inv_h);
  return t < 0.0f ? 0 : (t >= (float)n ? n - 1 : (int)t);
}

extern "C" {

int gq_cloud_check(int64_t n_obj, const int32_t* offsets_host, const float* radius_host, int64_t n_points,
                   int64_t queries_per_object) {
  GQ_REQUIRE(n_obj > 0 && n_obj < (1ll << 20), "cloud: n_obj must be in 1..2^20-1, got %lld", (long long)n_obj);
  GQ_REQUIRE(offsets_host && radius_host, "cloud: null offsets or radius");
  GQ_REQUIRE(offsets_host[0] == 0, "cloud: offsets must start at 0");
  for (int64_t i = 0; i < n_obj; ++i) {
    const int64_t N = (int64_t)offsets_host[i + 1] - offsets_host[i];
    GQ_REQUIRE(N >= 1 && N <= GQ_CLOUD_MAX_POINTS, "cloud: cloud %lld has N = %lld points, must be in 1..2^20", (long long)i,
               (long long)N);
    GQ_REQUIRE(radius_host[i] > 0.0f && radius_host[i] < GQ_INF_F, "cloud: radius rho of cloud %lld must be finite and > 0, got %g",
               (long long)i, (double)radius_host[i]);
  }
  GQ_REQUIRE(queries_per_object > 0, "cloud: queries_per_object must be > 0, got %lld", (long long)queries_per_object);
  GQ_REQUIRE(n_points == n_obj * queries_per_object, "cloud: n_points = %lld is not n_obj * queries_per_object = %lld * %lld",
             (long long)n_points, (long long)n_obj, (long long)queries_per_object);
  return GQ_OK;
}

int gq_cloudset_create(const float* points_host, const float* normals_host, const int32_t* offsets_host,
                       const float* radius_host, int n_obj, gqCloudSet** out) {
  GQ_REQUIRE(points_host && normals_host && out, "cloudset_create: null pointer");
  int rc = gq_cloud_check(n_obj, offsets_host, radius_host, n_obj, 1);  // no queries yet: one per object stands in
  if (rc) return rc;
  const int64_t total = offsets_host[n_obj];
  GQ_REQUIRE(total < (1ll << 31), "cloudset_create: too many points in all (%lld)", (long long)total);
  std::vector<float> nrm((size_t)total * 3);
  for (int64_t i = 0; i < total; ++i) {  // unit normals, normalised in double
    const double a = normals_host[i * 3], b = normals_host[i * 3 + 1], c = normals_host[i * 3 + 2];
    const double len = sqrt(a * a + b * b + c * c);
    GQ_REQUIRE(len > 0.0 && len < (double)GQ_INF_F, "cloudset_create: normal %lld is zero or not finite", (long long)i);
    nrm[i * 3] = (float)(a / len), nrm[i * 3 + 1] = (float)(b / len), nrm[i * 3 + 2] = (float)(c / len);
    for (int k = 0; k < 3; ++k)
      GQ_REQUIRE(fabsf(points_host[i * 3 + k]) < GQ_INF_F, "cloudset_create: point %lld is not finite", (long long)i);
  }
  std::vector<GqCloud> clouds(n_obj);
  std::vector<float4> pts(total), nrs(total);
  std::vector<int32_t> cell_start;
  std::vector<std::pair<int32_t, int32_t>> keys;  // (cell, index within the cloud)
  std::vector<uint8_t> mark;
  static const int steps[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128};
  for (int m = 0; m < n_obj; ++m) {
    const int64_t a = offsets_host[m], b = offsets_host[m + 1], N = b - a;
    GqCloud c{};
    float ext = 0.0f;
    for (int k = 0; k < 3; ++k) {
      float lo = points_host[a * 3 + k], hi = lo;
      for (int64_t i = a; i < b; ++i) {
        const float v = points_host[i * 3 + k];
        lo = v < lo ? v : lo, hi = v > hi ? v : hi;
      }
      c.lo[k] = lo, c.hi[k] = hi;
      ext = hi - lo > ext ? hi - lo : ext;
    }
    c.rho = radius_host[m];
    // one cell width for all axes: the coarsest of the steps that leaves at most 4 points per occupied cell on average,
    // with at most 8 N cells in all; a cloud without extent is one cell of width rho
    for (int si = 0; si < (int)(sizeof(steps) / sizeof(steps[0])); ++si) {
      const int g = ext > 0.0f ? steps[si] : 1;
      const float h = ext > 0.0f ? ext / (float)g : c.rho, inv_h = 1.0f / h;
      int n[3];
      for (int k = 0; k < 3; ++k) {
        const int want = (int)floorf((c.hi[k] - c.lo[k]) * inv_h) + 1;
        n[k] = want < 1 ? 1 : (want > g ? g : want);
      }
      const int64_t cells = (int64_t)n[0] * n[1] * n[2];
      if (si > 0 && cells > std::max<int64_t>(64, 8 * N)) break;  // keep the previous step
      c.h = h, c.inv_h = inv_h, c.n[0] = n[0], c.n[1] = n[1], c.n[2] = n[2];
      if (ext <= 0.0f) break;
      mark.assign((size_t)cells, 0);
      int64_t occupied = 0;
      for (int64_t i = a; i < b; ++i) {
        const int ix = gq_cloud_cell_(points_host[i * 3], c.lo[0], inv_h, n[0]), iy = gq_cloud_cell_(points_host[i * 3 + 1], c.lo[1], inv_h, n[1]),
                  iz = gq_cloud_cell_(points_host[i * 3 + 2], c.lo[2], inv_h, n[2]);
        uint8_t& f = mark[((size_t)iz * n[1] + iy) * n[0] + ix];
        occupied += !f;
        f = 1;
      }
      if (N <= 4 * occupied) break;
    }
    const int64_t cells = (int64_t)c.n[0] * c.n[1] * c.n[2];
    GQ_REQUIRE((int64_t)cell_start.size() + cells + 1 < (1ll << 31), "cloudset_create: cell tables too large");
    keys.clear();
    for (int64_t i = a; i < b; ++i) {
      const int ix = gq_cloud_cell_(points_host[i * 3], c.lo[0], c.inv_h, c.n[0]), iy = gq_cloud_cell_(points_host[i * 3 + 1], c.lo[1], c.inv_h, c.n[1]),
                iz = gq_cloud_cell_(points_host[i * 3 + 2], c.lo[2], c.inv_h, c.n[2]);
      keys.emplace_back((int32_t)(((int64_t)iz * c.n[1] + iy) * c.n[0] + ix), (int32_t)(i - a));
    }
    std::sort(keys.begin(), keys.end());  // by cell, then by original index
    c.cell_off = (int32_t)cell_start.size();
    c.pt_off = (int32_t)a, c.pt_end = (int32_t)b;
    cell_start.resize(cell_start.size() + cells + 1);
    int32_t* cs = cell_start.data() + c.cell_off;
    int64_t k = 0;
    for (int64_t cell = 0; cell <= cells; ++cell) {
      while (k < N && keys[k].first < cell) ++k;
      cs[cell] = (int32_t)(a + k);
    }
    for (int64_t i = 0; i < N; ++i) {
      const int64_t src = a + keys[i].second;
      union { int32_t i; float f; } idx;
      idx.i = keys[i].second;
      pts[a + i] = make_float4(points_host[src * 3], points_host[src * 3 + 1], points_host[src * 3 + 2], idx.f);
      nrs[a + i] = make_float4(nrm[src * 3], nrm[src * 3 + 1], nrm[src * 3 + 2], 0.0f);
    }
    clouds[m] = c;
  }
  auto cs = std::make_unique<gqCloudSet>();
  GqOwner& mem = cs->mem;
  cs->n_obj = n_obj;
  cs->off_host = mem.host_copy(offsets_host, (size_t)n_obj + 1);
  cs->rho_host = mem.host_copy(radius_host, (size_t)n_obj);
  cs->clouds = mem.upload(clouds.data(), clouds.size());
  cs->pts = mem.upload(pts.data(), pts.size());
  cs->nrm = mem.upload(nrs.data(), nrs.size());
  cs->cell_start = mem.upload(cell_start.data(), cell_start.size());
  if (mem.rc) return mem.rc;
  *out = cs.release();  // hipMemcpy from pageable memory has completed on return: nothing to wait for
  return GQ_OK;
}

int gq_cloudset_destroy(gqCloudSet* cs) {
  delete cs;
  return GQ_OK;
}

int gq_cloud_forward(const gqCloudSet* cs, const float* points, int64_t n_points, int64_t queries_per_object, float* dist_sq,
                     int32_t* sign, float* normal, float* closest, void* stream) {
  GQ_REQUIRE(cs, "cloud_forward: null cloud set");
  const int rc = gq_cloud_check(cs->n_obj, cs->off_host, cs->rho_host, n_points, queries_per_object);
  if (rc) return rc;
  GQ_REQUIRE(points && dist_sq && sign && closest, "cloud_forward: null pointer");
  GQ_REQUIRE(n_points < (1ll << 31), "cloud_forward: too many queries (%lld)", (long long)n_points);
  GqCloudArgs a{};
  a.clouds = cs->clouds, a.pts = cs->pts, a.nrm = cs->nrm, a.cell_start = cs->cell_start;
  a.points = points, a.N = n_points, a.qpo = queries_per_object;
  a.dist_sq = dist_sq, a.sign = sign, a.normal = normal, a.closest = closest;
  hipLaunchKernelGGL(gq_cloud_wave_kernel, dim3((unsigned)((n_points + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
