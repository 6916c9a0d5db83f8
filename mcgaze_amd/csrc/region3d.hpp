// What attend.hip (gaze targets, 3-D) and surface.hip (surface heat map) share: when a planar region of the PolyRegions3D tables is USABLE,
// its normal, the axis that is dropped, and the even-odd INSIDE test in the two coordinates left.  The arithmetic is stated once, in
// include/mcgaze_hip.h ("gaze targets, 3-D", REGIONS): double, uncontracted, every product and difference rounded on its own.
#pragma once
#include "common.hpp"

struct region3d {
  bool usable;
  int start, count, axis;                                        // the first vertex, their number, the dropped axis
  double v0x, v0y, v0z, Nx, Ny, Nz;
};

// Region j of (xyz f32 [num_vertices][3], region_start int32 [m + 1]), j < m.  The offsets are checked BEFORE the first vertex load: whatever
// the words hold, nothing outside xyz[0 .. num_vertices) is read.  Of a region that is not usable only `usable` means anything.
__device__ __forceinline__ region3d region3d_load(const float* __restrict__ xyz, int num_vertices, const int32_t* __restrict__ region_start, int j) {
#pragma clang fp contract(off)
  region3d r;
  r.usable = false;
  r.start = r.count = r.axis = 0;
  r.v0x = r.v0y = r.v0z = r.Nx = r.Ny = r.Nz = 0.0;
  const int s = region_start[j], e = region_start[j + 1];        // (j + 1 <= m: the table has m + 1 words)
  const int c = 0 <= s && s <= e && e <= num_vertices ? e - s : 0;              // (whatever the words hold, the difference cannot overflow)
  bool ok = c >= 3 && c <= MCG_ATTEND_POLY_VERTS;
  if (ok) {                                                      // every vertex below lies inside xyz[0 .. num_vertices)
    const float* v = xyz + 3 * (size_t)s;
    for (int k = 0; k < 3 * c; ++k) ok = ok && isfinite(v[k]);
    if (ok) {
      const double v0x = v[0], v0y = v[1], v0z = v[2];
      const double e1x = (double)v[3] - v0x, e1y = (double)v[4] - v0y, e1z = (double)v[5] - v0z;
      const double e2x = (double)v[6] - v0x, e2y = (double)v[7] - v0y, e2z = (double)v[8] - v0z;
      const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
      const double ax = fabs(Nx), ay = fabs(Ny), az = fabs(Nz);
      ok = !(Nx == 0.0 && Ny == 0.0 && Nz == 0.0);
      r.Nx = Nx, r.Ny = Ny, r.Nz = Nz;
      r.v0x = v0x, r.v0y = v0y, r.v0z = v0z;
      r.start = s;
      r.count = c;
      r.axis = ax >= ay && ax >= az ? 0 : ay >= az ? 1 : 2;     // the dropped axis: the largest |N|, the first on ties
    }
  }
  r.usable = ok;
  return r;
}

// P inside the polygon of the cnt vertices at v (a usable region's: v = xyz + 3 * start) by the even-odd rule in the two coordinates left
// after `axis` is dropped, edges in ascending order.  Where v and cnt are the same in every lane every load is one broadcast; the previous
// vertex is carried in registers.
__device__ __forceinline__ bool region3d_inside(const float* __restrict__ v, int cnt, int axis, double Px, double Py, double Pz) {
#pragma clang fp contract(off)
  const int iu = axis == 0 ? 1 : 0, iv = axis == 2 ? 1 : 2;
  const double pu = axis == 0 ? Py : Px, pv = axis == 2 ? Py : Pz;
  const double fu = v[iu], fv = v[iv];
  double au = fu, av = fv;
  bool inside = false;
  for (int k = 1; k <= cnt; ++k) {                               // edge k - 1: a = v[k - 1] -> b = v[k mod cnt]
    const double bu = k < cnt ? (double)v[3 * k + iu] : fu, bv = k < cnt ? (double)v[3 * k + iv] : fv;
    if ((av > pv) != (bv > pv) && pu < au + ((pv - av) * (bu - au)) / (bv - av)) inside = !inside;
    au = bu;
    av = bv;
  }
  return inside;
}
