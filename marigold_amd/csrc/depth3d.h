// The rules of depth to 3D (include/marigold_hip.h states them), one copy for points.hip, mesh.hip and view.hip: which pixels
// are usable, which are joined, a pixel's point, its tangents and its normal, the coefficients, a cell's split and faces, and what every entry point refuses about
// the map, the camera and the rules.  fp64 throughout; all three files are built with -ffp-contract=off, so every product, sum and quotient
// below is rounded on its own, in the order the header writes them.
#pragma once
#include <cmath>

#include "common.h"

namespace {

constexpr long long DEPTH3D_MAX_N = 1ll << 30;

struct PointsArgs {
  const float* d;
  const unsigned char* mask;   // or null
  const double* coef;          // or null
  int h, w;
  double fx, fy, cx, cy, z_min, z_max, edge_rel;
  int frame;
};

struct Vec3 {
  double x, y, z;
};

enum { EAST = 0, WEST = 1, SOUTH = 2, NORTH = 3 };

struct Pixel {
  bool usable;
  bool kept;        // usable, and joined to every usable 4-neighbour
  int x, y;
  double z;
  double zn[4];     // the neighbours' depths, where joined
  bool joined[4];   // the neighbour is usable and joined to this pixel
};

// the depth of an in-bounds pixel -> whether it is usable
__device__ __forceinline__ bool depth_at(const PointsArgs& a, double s, double t, int y, int x, double& z) {
  const long long i = (long long)y * a.w + x;
  if (a.mask != nullptr && a.mask[i] == 0) return false;
  const float d = a.d[i];
  z = (double)d;
  if (a.coef != nullptr) z = z * s + t;
  return isfinite(d) && isfinite(z) && z > a.z_min && z <= a.z_max;
}

__device__ __forceinline__ bool joined_to(const PointsArgs& a, double zp, double zq) {
  return a.edge_rel == 0.0 || fabs(zp - zq) <= a.edge_rel * fmin(zp, zq);
}

__device__ __forceinline__ Pixel classify(const PointsArgs& a, double s, double t, long long i) {
  Pixel p;
  p.y = (int)(i / a.w);
  p.x = (int)(i - (long long)p.y * a.w);
  p.usable = depth_at(a, s, t, p.y, p.x, p.z);
  p.kept = p.usable;
  const int nx[4] = {p.x + 1, p.x - 1, p.x, p.x}, ny[4] = {p.y, p.y, p.y + 1, p.y - 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p.joined[k] = false;
    p.zn[k] = 0.0;
    if (!p.usable || nx[k] < 0 || nx[k] >= a.w || ny[k] < 0 || ny[k] >= a.h) continue;
    double zq;
    if (!depth_at(a, s, t, ny[k], nx[k], zq)) continue;   // a neighbour that is not usable does not count against the pixel
    if (joined_to(a, p.z, zq)) {
      p.joined[k] = true;
      p.zn[k] = zq;
    } else {
      p.kept = false;
    }
  }
  return p;
}

__device__ __forceinline__ Vec3 point_of(const PointsArgs& a, int x, int y, double z) {
  return {(((double)x - a.cx) * z) / a.fx, (((double)y - a.cy) * z) / a.fy, z};
}

__device__ __forceinline__ Vec3 sub(const Vec3& a, const Vec3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

__device__ __forceinline__ double dot(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the tangent along one axis: `hi` the neighbour at the larger coordinate (east, south), `lo` the other
__device__ __forceinline__ bool tangent(const PointsArgs& a, const Pixel& p, const Vec3& P, int hi, int lo, int dx, int dy, Vec3& T) {
  if (!p.joined[hi] && !p.joined[lo]) return false;
  const Vec3 A = p.joined[hi] ? point_of(a, p.x + dx, p.y + dy, p.zn[hi]) : P;
  const Vec3 B = p.joined[lo] ? point_of(a, p.x - dx, p.y - dy, p.zn[lo]) : P;
  T = sub(A, B);
  return true;
}

// the normal of a pixel from its joined neighbours, in the frame asked for -> whether it has one
__device__ __forceinline__ bool normal_of(const PointsArgs& a, const Pixel& p, const Vec3& P, Vec3& N) {
  Vec3 Tu, Tv;
  if (!tangent(a, p, P, EAST, WEST, 1, 0, Tu) || !tangent(a, p, P, SOUTH, NORTH, 0, 1, Tv)) return false;
  N = {Tv.y * Tu.z - Tv.z * Tu.y, Tv.z * Tu.x - Tv.x * Tu.z, Tv.x * Tu.y - Tv.y * Tu.x};
  if (dot(N, P) > 0.0) N = {-N.x, -N.y, -N.z};
  const double nn = dot(N, N);
  if (!(nn > 0.0) || !isfinite(nn)) return false;
  const double len = sqrt(nn);
  N = {N.x / len, N.y / len, N.z / len};
  if (a.frame == 1) N = {N.x, -N.y, -N.z};
  return true;
}

__device__ __forceinline__ void load_coef(const PointsArgs& a, double& s, double& t) {
  s = 1.0;
  t = 0.0;
  if (a.coef != nullptr) {
    s = a.coef[0];
    t = a.coef[1];
  }
}

// ---- the cell rules of the meshes (6i) and the views (6j) ----

// A cell's code: bits 0 and 1 - T0, T1 are faces; bits 2.. - the form, which names the candidates' corners.
enum { FORM_SPLIT_AD = 0, FORM_SPLIT_BC = 1, FORM_NO_D = 2, FORM_NO_A = 3, FORM_NO_B = 4, FORM_NO_C = 5 };
enum { CORNER_A = 0, CORNER_B = 1, CORNER_C = 2, CORNER_D = 3 };

// the corners of candidate `slot` of a cell of `form`, two bits each, P0 lowest: (A, C, D), (A, D, B), (A, C, B), (B, C, D)
constexpr unsigned TRI_ACD = CORNER_A | CORNER_C << 2 | CORNER_D << 4, TRI_ADB = CORNER_A | CORNER_D << 2 | CORNER_B << 4;
constexpr unsigned TRI_ACB = CORNER_A | CORNER_C << 2 | CORNER_B << 4, TRI_BCD = CORNER_B | CORNER_C << 2 | CORNER_D << 4;

__device__ __forceinline__ unsigned triangle_of(int form, int slot) {
  switch (form) {
    case FORM_SPLIT_AD: return slot == 0 ? TRI_ACD : TRI_ADB;
    case FORM_SPLIT_BC: return slot == 0 ? TRI_ACB : TRI_BCD;
    case FORM_NO_D: return TRI_ACB;
    case FORM_NO_A: return TRI_BCD;
    case FORM_NO_B: return TRI_ACD;
    default: return TRI_ADB;   // FORM_NO_C
  }
}

// the code of the cell anchored at pixel i (0 for a pixel of the last row or column: no cell)
__device__ __forceinline__ unsigned cell_code(const PointsArgs& a, double s, double t, long long i) {
  const int y = (int)(i / a.w), x = (int)(i - (long long)y * a.w);
  if (x >= a.w - 1 || y >= a.h - 1) return 0;
  double z[4];
  bool ok[4];
  ok[CORNER_A] = depth_at(a, s, t, y, x, z[CORNER_A]);
  ok[CORNER_B] = depth_at(a, s, t, y, x + 1, z[CORNER_B]);
  ok[CORNER_C] = depth_at(a, s, t, y + 1, x, z[CORNER_C]);
  ok[CORNER_D] = depth_at(a, s, t, y + 1, x + 1, z[CORNER_D]);
  const int usable = (int)ok[0] + (int)ok[1] + (int)ok[2] + (int)ok[3];
  if (usable < 3) return 0;
  int form, slots = 1;
  if (usable == 4) {
    form = fabs(z[CORNER_A] - z[CORNER_D]) <= fabs(z[CORNER_B] - z[CORNER_C]) ? FORM_SPLIT_AD : FORM_SPLIT_BC;
    slots = 2;
  } else {
    form = !ok[CORNER_D] ? FORM_NO_D : !ok[CORNER_A] ? FORM_NO_A : !ok[CORNER_B] ? FORM_NO_B : FORM_NO_C;
  }
  unsigned code = (unsigned)form << 2;
#pragma unroll
  for (int slot = 0; slot < 2; ++slot) {
    if (slot >= slots) continue;
    const unsigned tri = triangle_of(form, slot);
    const double z0 = z[tri & 3u], z1 = z[(tri >> 2) & 3u], z2 = z[(tri >> 4) & 3u];   // (usable corners only: the form saw to that)
    if (joined_to(a, z0, z1) && joined_to(a, z1, z2) && joined_to(a, z2, z0)) code |= 1u << slot;
  }
  return code;
}

// what every call refuses about the map, the camera and the rules -> 0 | 2 with the message set
inline int check_common(const char* fn, int h, int w, double fx, double fy, double cx, double cy, double z_min, double z_max, double edge_rel,
                        int normals_frame) {
  MG_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= DEPTH3D_MAX_N, "%s: a map of %d x %d, 1 to 2^30 pixels are supported", fn, h, w);
  MG_REQUIRE(std::isfinite(fx) && fx > 0.0 && std::isfinite(fy) && fy > 0.0, "%s: the focal lengths (%g, %g) are not finite and > 0", fn, fx, fy);
  MG_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "%s: the principal point (%g, %g) is not finite", fn, cx, cy);
  MG_REQUIRE(std::isfinite(z_min) && z_min >= 0.0, "%s: z_min %g is not finite and >= 0", fn, z_min);
  MG_REQUIRE(z_max > z_min, "%s: z_max %g is not above z_min %g", fn, z_max, z_min);   // (false for a NaN)
  MG_REQUIRE(std::isfinite(edge_rel) && edge_rel >= 0.0, "%s: edge_rel %g is not finite and >= 0", fn, edge_rel);
  MG_REQUIRE(normals_frame == MG_NORMALS_FRAME_CAMERA || normals_frame == MG_NORMALS_FRAME_MARIGOLD, "%s: unknown normals frame %d", fn,
             normals_frame);
  return 0;
}

}  // namespace
