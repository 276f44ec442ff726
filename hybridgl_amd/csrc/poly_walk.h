// The boundary walk of a polygon (refer/external/maskApi.c:161-196 rleFrPoly; gtmask.cpp polygon_crossings is its sequential
// host form and the yardstick), written so that every step stands alone: plain functions that compile under g++ (the sanitizer
// harness tests/native/poly_walk_sanitize.cpp) and as __device__ code (rle_poly.hip).  Nothing here needs HIP when __HIPCC__ is
// absent.
//
// The sequential codec pushes the points of all edges into one list and looks at every pair of neighbours.  Here a point is
// (edge j, step d): edge j runs from vertex j to vertex (j + 1) % k on the 5x grid, d = 0 .. n_j along its major axis in the
// edge's own direction.  The predecessor of (j, d > 0) is (j, d - 1); the predecessor of (j, 0) is the LAST point of edge j - 1,
// computed by that edge's formula -- not the shared vertex: with a negative coordinate (int)(xs + slope*n + 0.5) truncates
// towards zero and may miss xe, and the sequential codec compares against what it computed.  (0, 0) has no predecessor.
//
// Two hazards, settled here:
//   Contraction.  The .hip files are built with -ffp-contract=on, the host codec with off; ys + slope*t + 0.5 and 5*x + 0.5 must
//   round twice.  Every function that holds such an expression starts with `#pragma clang fp contract(off)`, which binds
//   whatever the command line says (hipcc is clang).  g++ does not know the pragma and is not given it: the harness is built with
//   -ffp-contract=off, and baseline x86-64 has no fused instruction to contract into.
//   The degenerate edge (both ends on one grid point: dx = dy = 0, one point).  The host's slope is 0/0 and its point's v is
//   (int)NaN, whatever the machine makes of that (INT_MIN on x86).  Here the point is the grid point itself, no division.  Its v
//   cannot reach an emitted crossing: a crossing needs u to differ between the two points of a pair, the degenerate point's u is
//   the vertex's x exactly, and both neighbours are points AT that vertex: the end of edge j - 1 and the start of edge j + 1.
//   Their u is the vertex's x when their edge is x-major (u = t + xs, integers) and (int)(X + 0.5) with X within an ulp of x when
//   it is y-major: x again for x >= 0, x + 1 for x < 0.  So u differs only at a negative x, the pair's column is
//   min(u0, u1) = x < 0, and such a crossing is dropped before v is read.
#ifndef HGL_POLY_WALK_H
#define HGL_POLY_WALK_H
#include <math.h>

#ifdef __HIPCC__
#define POLY_FN static __host__ __device__ inline
#else
#define POLY_FN static inline
#endif
#if defined(__clang__)
#define POLY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define POLY_NO_CONTRACT
#endif

// the host codec's guard: the walk is 5 steps per pixel, keep it finite and the int casts defined
POLY_FN bool poly_coord_ok(double c) { return c == c && c > -1.0e5 && c < 1.0e5; }

// vertex coordinate -> 5x grid
POLY_FN int poly_grid(double c) {
  POLY_NO_CONTRACT
  return (int)(5.0 * c + 0.5);
}

// an edge on the grid, from (xs, ys) on: its ends swapped where the codec swaps them, n + 1 points
struct PolyEdge {
  int xs, ys, n;
  bool x_major, flip, point;      // point: the degenerate edge
  double slope;
};

POLY_FN PolyEdge poly_edge(int xs, int ys, int xe, int ye) {
  PolyEdge e;
  const int dx = xe > xs ? xe - xs : xs - xe, dy = ye > ys ? ye - ys : ys - ye;
  e.x_major = dx >= dy;
  e.flip = (e.x_major && xs > xe) || (!e.x_major && ys > ye);
  if (e.flip) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  e.xs = xs;
  e.ys = ys;
  e.n = e.x_major ? dx : dy;
  e.point = e.n == 0;      // dx >= dy and dx == 0
  e.slope = e.point ? 0.0 : (e.x_major ? (double)(ye - ys) / dx : (double)(xe - xs) / dy);
  return e;
}

// edge j of a polygon of k vertices xy = x0,y0,x1,y1,...
POLY_FN PolyEdge poly_edge_of(const double* xy, int k, int j) {
  const int a = j, b = j + 1 < k ? j + 1 : 0;
  return poly_edge(poly_grid(xy[2 * a]), poly_grid(xy[2 * a + 1]), poly_grid(xy[2 * b]), poly_grid(xy[2 * b + 1]));
}

// the walk point of (edge, step d), d = 0 .. e.n
POLY_FN void poly_point(const PolyEdge& e, int d, int* u, int* v) {
  POLY_NO_CONTRACT
  if (e.point) { *u = e.xs; *v = e.ys; return; }
  const int t = e.flip ? e.n - d : d;
  if (e.x_major) { *u = t + e.xs; *v = (int)(e.ys + e.slope * t + 0.5); }
  else { *v = t + e.ys; *u = (int)(e.xs + e.slope * t + 0.5); }
}

// the predecessor of (edge j, step d) in the polygon's walk; false: (0, 0) has none
POLY_FN bool poly_pred(const double* xy, int k, int j, const PolyEdge& e, int d, int* u, int* v) {
  if (d > 0) { poly_point(e, d - 1, u, v); return true; }
  if (j == 0) return false;
  const PolyEdge p = poly_edge_of(xy, k, j - 1);
  poly_point(p, p.n, u, v);
  return true;
}

// the crossing of two consecutive walk points (u0, v0) -> (u1, v1): true when the fill toggles, *pos = x*H + y in [0, H*W]
// (H*W itself toggles nothing inside the image)
POLY_FN bool poly_crossing(int u0, int v0, int u1, int v1, int H, int W, unsigned* pos) {
  POLY_NO_CONTRACT
  if (u1 == u0) return false;
  double xd = (double)(u1 < u0 ? u1 : u1 - 1);
  xd = (xd + 0.5) / 5.0 - 0.5;
  if (floor(xd) != xd || xd < 0 || xd > W - 1) return false;
  double yd = (double)(v1 < v0 ? v1 : v0);
  yd = (yd + 0.5) / 5.0 - 0.5;
  if (yd < 0) yd = 0; else if (yd > H) yd = H;
  yd = ceil(yd);
  *pos = (unsigned)((int)xd * H + (int)yd);
  return true;
}

// (edge j, step d) -> does it toggle, and where: everything a thread needs of one step
POLY_FN bool poly_step(const double* xy, int k, int j, const PolyEdge& e, int d, int H, int W, unsigned* pos) {
  int u0, v0, u1, v1;
  if (!poly_pred(xy, k, j, e, d, &u0, &v0)) return false;
  poly_point(e, d, &u1, &v1);
  return poly_crossing(u0, v0, u1, v1, H, W, pos);
}

#endif  // HGL_POLY_WALK_H
