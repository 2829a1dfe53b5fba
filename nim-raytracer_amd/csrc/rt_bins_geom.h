// rt_bins_geom.h — float64 geometry shared by the host bin builders
// (rt_bins.cpp, the tests' reference) and the per-frame device builders
// (rt_frame.hip). Both are compiled with -ffp-contract=off, so host and
// device form every bound with the same roundings and build the same lists.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include "rt_common.h"

namespace rtmi {
namespace bg {

// glm column-major: m[c*4 + r]
__host__ __device__ inline void xform_point(const double m[16], const double p[3], double out[3]) {
  for (int r = 0; r < 3; ++r) out[r] = m[0 * 4 + r] * p[0] + m[1 * 4 + r] * p[1] + m[2 * 4 + r] * p[2] + m[3 * 4 + r];
}
__host__ __device__ inline void xform_dir(const double m[16], const double d[3], double out[3]) {
  for (int r = 0; r < 3; ++r) out[r] = m[0 * 4 + r] * d[0] + m[1 * 4 + r] * d[1] + m[2 * 4 + r] * d[2];
}
__host__ __device__ inline double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ inline void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline double norm3(const double a[3]) { return sqrt(dot3(a, a)); }
__host__ __device__ inline double dmin(double a, double b) { return b < a ? b : a; }
__host__ __device__ inline double dmax(double a, double b) { return a < b ? b : a; }

// The single-sided test rejects det < 1e-6 (geom.nim:306). det is computed
// in float32 from the object-space direction rd and nn = -(e1 x e2); a face
// is left out of a family's bins only when det stays below 1e-6 even with a
// float32 error of 1e-6 * |rd| * |nn| (generous: the test's own rounding is
// ~1e-7 of that).
__host__ __device__ inline bool never_passes(double det_upper, double rd_max, double nlen) {
  return det_upper + 1e-6 * rd_max * nlen < 1e-6;
}

// Separating-axis test of a 2D triangle q[0..5] (x, y pairs) against the box
// [x0, x1] x [y0, y1] (the box axes are the caller's bounding-rectangle
// loop): false only when one triangle edge has all four box corners strictly
// outside it.
__host__ __device__ inline bool tri_meets_box(const double* q, double x0, double y0, double x1, double y1) {
  const double area = (q[2] - q[0]) * (q[5] - q[1]) - (q[3] - q[1]) * (q[4] - q[0]);
  if (!(area != 0.0)) return true;  // degenerate (or NaN): keep
  const double sg = area > 0.0 ? 1.0 : -1.0;
  const double cx[4] = {x0, x1, x0, x1}, cy[4] = {y0, y0, y1, y1};
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1;
    const double ax = q[2 * k], ay = q[2 * k + 1];
    const double bx = q[2 * k1], by = q[2 * k1 + 1];
    double best = -INFINITY;
    for (int c = 0; c < 4; ++c) best = dmax(best, sg * ((bx - ax) * (cy[c] - ay) - (by - ay) * (cx[c] - ax)));
    if (best < 0.0) return false;
  }
  return true;
}

// ---- light grids (rt_bins.cpp build_light_grid, rt_lights_gpu.hip) ---------
//
// The host builder and the device builder of a distant light's grid call the
// same functions below, so every bound, cell range and coverage is the same
// float64 value on both sides and the two build the same arrays.

// Area of the 2D triangle q[0..5] (x, y pairs) inside the box [x0, x1] x
// [y0, y1]: Sutherland-Hodgman against the four edges, then the shoelace.
__host__ __device__ inline double clipped_area(const double* q, double x0, double y0, double x1, double y1) {
  double a[16][2], b[16][2];
  int n = 3;
  for (int k = 0; k < 3; ++k) {
    a[k][0] = q[2 * k];
    a[k][1] = q[2 * k + 1];
  }
  // edge e: keep points with s * p[axis] <= s * lim
  const int axis[4] = {0, 0, 1, 1};
  const double lim[4] = {x0, x1, y0, y1}, sgn[4] = {-1.0, 1.0, -1.0, 1.0};
  for (int ei = 0; ei < 4 && n > 0; ++ei) {
    const int ax = axis[ei];
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const double* P = a[k];
      const double* Q = a[(k + 1) % n];
      const double dp = sgn[ei] * (P[ax] - lim[ei]), dq = sgn[ei] * (Q[ax] - lim[ei]);
      if (dp <= 0.0) {
        b[m][0] = P[0];
        b[m][1] = P[1];
        ++m;
      }
      if ((dp < 0.0 && dq > 0.0) || (dp > 0.0 && dq < 0.0)) {
        const double t = dp / (dp - dq);
        b[m][0] = P[0] + t * (Q[0] - P[0]);
        b[m][1] = P[1] + t * (Q[1] - P[1]);
        ++m;
      }
    }
    n = m;
    for (int k = 0; k < n; ++k) {
      a[k][0] = b[k][0];
      a[k][1] = b[k][1];
    }
  }
  double area = 0.0;
  for (int k = 0; k < n; ++k) {
    const double* P = a[k];
    const double* Q = a[(k + 1) % n];
    area += P[0] * Q[1] - Q[0] * P[1];
  }
  return 0.5 * fabs(area);
}

// A distant light as its grid sees it: the object-space shadow direction rd
// (the kernel's rd, up to float32 rounding), its length, and an orthonormal
// basis (e1, e2) of the plane orthogonal to it. dir: the light's travel
// direction (world); false: a degenerate direction (no grid).
struct LightBasis {
  double rd[3], rlen, e1[3], e2[3];
};
__host__ __device__ inline bool light_basis(const double w2o[16], const double dir[3], LightBasis* b) {
  const double sd[3] = {-dir[0], -dir[1], -dir[2]};
  xform_dir(w2o, sd, b->rd);
  b->rlen = norm3(b->rd);
  if (!(b->rlen > 0.0) || !isfinite(b->rlen)) return false;
  const double u[3] = {b->rd[0] / b->rlen, b->rd[1] / b->rlen, b->rd[2] / b->rlen};
  // the axis u is least aligned with (ties: x before y before z)
  const int ax = fabs(u[0]) <= fabs(u[1]) && fabs(u[0]) <= fabs(u[2]) ? 0 : fabs(u[1]) <= fabs(u[2]) ? 1 : 2;
  double a[3] = {0, 0, 0};
  a[ax] = 1.0;
  cross3(a, u, b->e1);
  const double l1 = norm3(b->e1);
  for (int k = 0; k < 3; ++k) b->e1[k] /= l1;
  cross3(u, b->e1, b->e2);
  return true;
}
// max(scale, |every coordinate of the face|): the grids' length scale starts at 1.
__host__ __device__ inline double light_face_scale(double scale, const double v[3][3]) {
  for (int a = 0; a < 3; ++a)
    for (int k = 0; k < 3; ++k) scale = dmax(scale, fabs(v[a][k]));
  return scale;
}
// One face under one light: false when it faces away from the light (never
// listed); else its projected vertices q[6] and their bounding box grown by
// delta (box: u0, u1, v0, v1).
__host__ __device__ inline bool light_face_box(const LightBasis& b, const double v[3][3], double delta, double q[6],
                                               double box[4]) {
  double f1[3], f2[3], c[3], nn[3];
  for (int k = 0; k < 3; ++k) {
    f1[k] = v[1][k] - v[0][k];
    f2[k] = v[2][k] - v[0][k];
  }
  cross3(f1, f2, c);
  for (int k = 0; k < 3; ++k) nn[k] = -c[k];
  if (never_passes(dot3(b.rd, nn), b.rlen, norm3(nn))) return false;
  double bu0 = INFINITY, bu1 = -INFINITY, bv0 = INFINITY, bv1 = -INFINITY;
  for (int a = 0; a < 3; ++a) {
    const double pu = dot3(v[a], b.e1), pv = dot3(v[a], b.e2);
    q[2 * a] = pu;
    q[2 * a + 1] = pv;
    bu0 = dmin(bu0, pu);
    bu1 = dmax(bu1, pu);
    bv0 = dmin(bv0, pv);
    bv1 = dmax(bv1, pv);
  }
  box[0] = bu0 - delta;
  box[1] = bu1 + delta;
  box[2] = bv0 - delta;
  box[3] = bv1 + delta;
  return true;
}
// The grid's header from the bounds of the kept faces' boxes: about `density`
// cells per listed face, square cells, at most 4096 per side; kept == 0: the
// empty 1 x 1 grid. off_base / ent_base are the caller's.
__host__ __device__ inline void light_grid_header(const LightBasis& b, double scale, long long kept, double umin,
                                                  double umax, double vmin, double vmax, double density,
                                                  LightGrid* g) {
  for (int k = 0; k < 3; ++k) {
    g->e1[k] = (float)b.e1[k];
    g->e2[k] = (float)b.e2[k];
  }
  g->rmax = (float)(100.0 * scale);
  if (kept == 0) {
    g->u0 = g->v0 = 0.0f;
    g->inv_h = 1.0f;
    g->gu = g->gv = 1;
    return;
  }
  const double du = dmax(umax - umin, 1e-30), dv = dmax(vmax - vmin, 1e-30);
  double h = sqrt(du * dv / (density * (double)kept));
  h = dmax(h, dmax(du, dv) / 4096.0);
  const int cu = (int)ceil(du / h), cv = (int)ceil(dv / h);
  // the float32 origin / cell size the kernel uses, so host and device agree on
  // cell edges up to float32 rounding (covered by delta)
  g->u0 = (float)umin;
  g->v0 = (float)vmin;
  g->inv_h = (float)(1.0 / h);
  g->gu = cu > 4096 ? 4096 : cu < 1 ? 1 : cu;
  g->gv = cv > 4096 ? 4096 : cv < 1 ? 1 : cv;
}
// The cells a face's grown box reaches (rc: c0, c1, r0, r1; empty when c0 > c1
// or r0 > r1).
__host__ __device__ inline void light_cell_range(const LightGrid& g, const double box[4], int rc[4]) {
  const double ih = (double)g.inv_h;
  const int c0 = (int)floor((box[0] - (double)g.u0) * ih), c1 = (int)floor((box[1] - (double)g.u0) * ih);
  const int r0 = (int)floor((box[2] - (double)g.v0) * ih), r1 = (int)floor((box[3] - (double)g.v0) * ih);
  rc[0] = c0 < 0 ? 0 : c0;
  rc[1] = c1 > g.gu - 1 ? g.gu - 1 : c1;
  rc[2] = r0 < 0 ? 0 : r0;
  rc[3] = r1 > g.gv - 1 ? g.gv - 1 : r1;
}
// Cell (c, r) grown by delta: a face is listed there when it meets this box.
__host__ __device__ inline bool light_face_in_cell(const LightGrid& g, const double* q, double delta, int c, int r) {
  const double ih = (double)g.inv_h;
  const double cu0 = (double)g.u0 + c / ih, cv0 = (double)g.v0 + r / ih;
  return tri_meets_box(q, cu0 - delta, cv0 - delta, cu0 + 1.0 / ih + delta, cv0 + 1.0 / ih + delta);
}
// The area of cell (c, r) a face's projection covers: a cell's faces are
// ordered by it, largest first (ties: the lower leaf index first).
__host__ __device__ inline double light_cell_cover(const LightGrid& g, const double* q, int c, int r) {
  const double hc = 1.0 / (double)g.inv_h;
  const double cu0 = (double)g.u0 + c * hc, cv0 = (double)g.v0 + r * hc;
  return clipped_area(q, cu0, cv0, cu0 + hc, cv0 + hc);
}

// LTri (rt_common.h) of face v for the shadow direction d (mesh object
// space, float64): p, q, tv rounded to float32 first, the constants formed
// from the ROUNDED vectors (u(v0) = 0 up to the float64 sum), so each affine
// function keeps its zero at the face's vertex.
__host__ __device__ inline void make_ltri(const double v[3][3], const double d[3], int32_t face, LTri* out) {
  double e1[3], e2[3], cr[3], nn[3], p[3], q[3], me1[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = v[1][k] - v[0][k];
    e2[k] = v[2][k] - v[0][k];
    me1[k] = -e1[k];
  }
  cross3(e1, e2, cr);
  for (int k = 0; k < 3; ++k) nn[k] = -cr[k];
  const double det = dot3(nn, d);
  const LTri zero = {};
  *out = zero;
  out->id = face;
  if (!(det >= 1e-6)) {  // geom.nim:306: never passes for this light
    out->cu = out->cv = out->ct = -1.0f;
    return;
  }
  cross3(d, e2, p);
  cross3(d, me1, q);
  double pr[3], qr[3], tr[3];
  for (int k = 0; k < 3; ++k) {
    out->p[k] = (float)(p[k] / det);
    out->q[k] = (float)(q[k] / det);
    out->tv[k] = (float)(nn[k] / -det);
    pr[k] = out->p[k];
    qr[k] = out->q[k];
    tr[k] = out->tv[k];
  }
  out->cu = (float)-dot3(pr, v[0]);
  out->cv = (float)-dot3(qr, v[0]);
  out->ct = (float)-dot3(tr, v[0]);
}
// The slot every light's record array starts from: a face that can never
// pass (u = v = t = -1). An all-zero record would read as a hit at t = 0.
__host__ __device__ inline LTri culled_ltri() {
  LTri c = {};
  c.cu = c.cv = c.ct = -1.0f;
  c.id = -1;
  return c;
}

// Camera-ray bins of one face (build_pixel_bins): the face's projected
// vertices in pixel coordinates (q[6]) and its pixel rectangle (rect[4]:
// x0, x1, y0, y1; x0 = -1: the face gets no bin). Returns false when a vertex
// lies at or behind the camera plane (no bins for this camera).
struct PixCam {
  double o2w[16], w2c[16];  // mesh object -> world, world -> camera
  double co[3];             // camera origin in mesh object space
  double rd_min, rd_max;    // |rd| bounds of a unit world direction in object space
  double cam_a, cam_c;      // the float32 kernel's camera constants (rtmi.cpp fill_fast)
  double margin;            // rt_bins.h kPixelMargin
  int width, height;
};
// The single-sided cull of a face for every camera ray (geom.nim:306): true
// when no camera ray reaching the face's plane can pass det >= 1e-6.
__host__ __device__ inline bool face_is_back(const PixCam& c, const double v[3][3]) {
  double e1[3], e2[3], cr[3], nn[3], dc[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = v[1][k] - v[0][k];
    e2[k] = v[2][k] - v[0][k];
    dc[k] = v[0][k] - c.co[k];
  }
  cross3(e1, e2, cr);
  for (int k = 0; k < 3; ++k) nn[k] = -cr[k];
  const double nlen = norm3(nn);
  // every camera ray reaching the face's plane has det = |rd| (v0 - C).nn / |P - C|
  const double s = dot3(dc, nn);
  double maxd = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double dv[3] = {v[a][0] - c.co[0], v[a][1] - c.co[1], v[a][2] - c.co[2]};
    maxd = dmax(maxd, norm3(dv));
  }
  return s <= 0.0 && maxd > 0.0 && never_passes(c.rd_min * s / maxd, c.rd_max, nlen);
}
// The face's projected vertices and grown pixel rectangle (rect[0] = -1:
// off screen); false when a vertex lies at or behind the camera plane.
__host__ __device__ inline bool face_project_rect(const PixCam& c, const double v[3][3], double q[6], int rect[4]) {
  rect[0] = rect[1] = rect[2] = rect[3] = -1;
  double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  for (int a = 0; a < 3; ++a) {
    double pw[3], pc[3];
    xform_point(c.o2w, v[a], pw);
    xform_point(c.w2c, pw, pc);
    if (!(pc[2] < -1e-9 * (1.0 + fabs(pc[0]) + fabs(pc[1])))) return false;
    const double px = 0.5 * c.width + (pc[0] / -pc[2]) / c.cam_a;
    const double py = 0.5 * c.height - (pc[1] / -pc[2]) / c.cam_c;
    q[2 * a] = px;
    q[2 * a + 1] = py;
    xmin = dmin(xmin, px);
    xmax = dmax(xmax, px);
    ymin = dmin(ymin, py);
    ymax = dmax(ymax, py);
  }
  const double m = c.margin;
  if (!(xmax + m >= 0.0 && ymax + m >= 0.0 && xmin - m < c.width && ymin - m < c.height)) return true;
  rect[0] = (int)dmax(0.0, floor(xmin - m));
  rect[1] = (int)dmin((double)c.width - 1, floor(xmax + m));
  rect[2] = (int)dmax(0.0, floor(ymin - m));
  rect[3] = (int)dmin((double)c.height - 1, floor(ymax + m));
  return true;
}
__host__ __device__ inline bool face_pixel_rect(const PixCam& c, const double v[3][3], double q[6], int rect[4]) {
  if (face_is_back(c, v)) {  // a back face: in no pixel's list
    rect[0] = rect[1] = rect[2] = rect[3] = -1;
    return true;
  }
  return face_project_rect(c, v, q, rect);
}

// Shadow skips (build_shadow_skips) of one pixel whose camera-ray list is
// empty: bit l set when every shadow ray to distant light l leaving a camera
// hit of the pixel provably meets no face. Per plane (a plane object of the
// scene, y = 0 in its object space), the per-camera constants:
struct SkipPlaneC {
  double oy;        // camera origin's object-space y
  double row[3];    // object-space y of a world direction: row . d
  double n[3];      // world normal (object_to_world * (0, 1, 0), as the kernel's N)
  double tol;       // float32 error allowance of row . d
};
// One light's grid as the skip test reads it: the float32 LightGrid values
// widened, and its occupancy prefix counts ((gu + 1) x (gv + 1)).
struct SkipGrid {
  double e1[3], e2[3], u0, v0, inv_h;
  int gu, gv;
  const int* sat;
};
struct SkipCam {
  double c2w[16], cw[3], mesh_w2o[16];
  double cam_a, cam_c, margin, bias;
  int width, height;
};
// The skip bits (a subset of `have`) shared by every pixel of the rectangle
// [x0, x1] x [y0, y1] — its grown corner rays bound every pixel's — or 0
// when a horizon crosses it. One pixel: x0 = x1, y0 = y1.
__host__ __device__ inline unsigned rect_skip_bits(const SkipCam& c, const SkipPlaneC* planes, int nplanes,
                                                   const SkipGrid* grids, int nl, unsigned have, int x0, int y0,
                                                   int x1, int y1) {
  double dw[4][3];
  for (int k = 0; k < 4; ++k) {
    const double px = (k & 1) ? x1 + 1 + c.margin : x0 - c.margin, py = (k & 2) ? y1 + 1 + c.margin : y0 - c.margin;
    const double dc[3] = {(px - 0.5 * c.width) * c.cam_a, (0.5 * c.height - py) * c.cam_c, -1.0};
    xform_dir(c.c2w, dc, dw[k]);
    const double il = 1.0 / norm3(dw[k]);
    for (int a = 0; a < 3; ++a) dw[k][a] *= il;
  }
  unsigned bits = have;
  for (int k = 0; k < nplanes && bits; ++k) {
    const SkipPlaneC& P = planes[k];
    int hit = 0, miss = 0;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < 4; ++q) {
      const double dy = dot3(P.row, dw[q]);
      // the kernel counts a plane hit at t = -oy / dy >= 0 with |dy| > 1e-6
      const double s = P.oy > 0.0 ? -dy : dy;  // > 0: towards the plane
      if (s > P.tol + 1e-6) {
        ++hit;
        t[q] = -P.oy / dy;
      } else if (s < -P.tol) {
        ++miss;
      }
    }
    if (miss == 4) continue;  // no ray of the pixel reaches this plane
    if (hit != 4) return 0u;  // a horizon inside the pixel: unbounded footprint
    for (int l = 0; l < nl; ++l) {
      if (!(bits >> l & 1u)) continue;
      const SkipGrid& g = grids[l];
      double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, qmax = 0.0;
      for (int q = 0; q < 4; ++q) {
        // shadow-ray origin: hit + N * bias (renderer.nim:94-101), in mesh space
        const double so[3] = {c.cw[0] + dw[q][0] * t[q] + P.n[0] * c.bias, c.cw[1] + dw[q][1] * t[q] + P.n[1] * c.bias,
                              c.cw[2] + dw[q][2] * t[q] + P.n[2] * c.bias};
        double o[3];
        xform_point(c.mesh_w2o, so, o);
        qmax = dmax(qmax, dmax(fabs(o[0]), dmax(fabs(o[1]), fabs(o[2]))));
        const double u = dot3(o, g.e1), v = dot3(o, g.e2);
        umin = dmin(umin, u);
        umax = dmax(umax, u);
        vmin = dmin(vmin, v);
        vmax = dmax(vmax, v);
      }
      // float32 hit points, transforms, shadow rays and triangle tests: far
      // inside 1e-4 of the magnitudes. A face a shadow ray of the footprint
      // can meet overlaps the grown footprint, so it is listed in a cell
      // the footprint's cell range holds (cells list every face whose grown
      // projection meets them): no cell beyond that range is needed.
#ifndef RTMI_SKIP_CELL_PAD
#define RTMI_SKIP_CELL_PAD 0.0
#endif
      const double mw = 1e-4 * (1.0 + qmax) + 1e-4 * fabs(c.bias);
      const double ih = g.inv_h;
      const double fu0 = (umin - mw - g.u0) * ih - RTMI_SKIP_CELL_PAD, fu1 = (umax + mw - g.u0) * ih + RTMI_SKIP_CELL_PAD;
      const double fv0 = (vmin - mw - g.v0) * ih - RTMI_SKIP_CELL_PAD, fv1 = (vmax + mw - g.v0) * ih + RTMI_SKIP_CELL_PAD;
      if (!(fu1 >= 0.0 && fv1 >= 0.0 && fu0 < g.gu && fv0 < g.gv)) continue;  // off the grid
      if (!isfinite(fu0 + fu1 + fv0 + fv1)) {
        bits &= ~(1u << l);
        continue;
      }
      const int u0 = (int)dmax(0.0, floor(fu0)), u1 = (int)dmin((double)g.gu - 1, floor(fu1));
      const int v0 = (int)dmax(0.0, floor(fv0)), v1 = (int)dmin((double)g.gv - 1, floor(fv1));
      const long long W1 = (long long)g.gu + 1;
      const int n = g.sat[(long long)(v1 + 1) * W1 + u1 + 1] - g.sat[(long long)v0 * W1 + u1 + 1] -
                    g.sat[(long long)(v1 + 1) * W1 + u0] + g.sat[(long long)v0 * W1 + u0];
      if (n != 0) bits &= ~(1u << l);
    }
  }
  return bits;
}
__host__ __device__ inline unsigned pixel_skip_bits(const SkipCam& c, const SkipPlaneC* planes, int nplanes,
                                                    const SkipGrid* grids, int nl, unsigned have, int x, int y) {
  return rect_skip_bits(c, planes, nplanes, grids, nl, have, x, y, x, y);
}

// ---- uniform lean pixels of the one-plane kernel (rt_fast.h lean1q_loop) --
//
// A lean pixel of a one-plane launch whose m x m samples provably all take
// the same branch of lean1q_loop is a fixed sum of one constant: every camera
// ray hits the plane and no shadow ray is occluded by it (uniform-lit, the
// constant is albedo x irradiance), or every camera ray misses (uniform-sky,
// the background). This is a proof about the kernel's FLOAT32 arithmetic, so
// it evaluates the kernel's own expressions from the kernel's own parameter
// values (FastParams), with fmaf exactly where the kernel has one.
//
// The kernel, per sample of column index i and row index j (0 .. m - 1):
//   px = x + fma(i, st, of)      cx = (px - cam_b) * cam_a
//   py = y + fma(j, st, of)      cy = (cam_d - py) * cam_c
//   N  = fma(cy, c7, fma(cx, c4, -c10))
//   rl = rsq(fma(cy, cy, fma(cx, cx, 1)))      dy = N * rl
//   t  = nroy * rcp(dy)
//   hit = |dy| > 1e-6 and t in [-0, +inf)      (class test: -0, +0, +denormal, +normal)
// Every step from i to N is a monotone function followed by a monotone
// rounding, and so is every step from j to N, and the direction does not
// depend on the other index (it is the sign of st cam_a c4, resp. of
// -st cam_c c7). So N over the pixel's samples lies between its values at the
// four corner samples (indices 0 and m - 1), which are evaluated here; cx^2
// and cy^2 are largest at an end of their ranges.
//
// Both rules need N finite and of one strict sign at the four corners, with
// |N| <= 1e10, and 1e-20 <= |nroy| <= 1e20. As rl <= 1 (its argument is >= 1;
// v_rsq is within 1 ulp), |dy| <= 1.0000003e10, so |t| >= 0.99e-30: t is a
// normal number, never a zero of either sign, and at most 1e26 when
// |dy| > 1e-6: finite.
//  * all miss: N and nroy of opposite signs. Then dy has N's sign or is 0
//    (rl = 0 when its argument overflows), and wherever |dy| > 1e-6, t is a
//    negative non-zero number or -inf: no hit. (No margin on |dy| is needed:
//    a sample below the threshold is a miss as well.)
//  * all hit: N and nroy of the same sign and |dy| > 1e-6 for every sample.
//    The lower bound: min |N| over the corners times 1 / sqrt(S), S = 1 +
//    max cx^2 + max cy^2 formed in float64 (products of floats are exact
//    there), against the kernel's float threshold with a relative margin of
//    1e-5. What the margin covers: the kernel's two roundings of S
//    (<= 2^-24 each on S, half of that on rl), v_rsq's 1 ulp (2^-23), the
//    product's rounding (2^-24) and this bound's own float64 roundings
//    (~1e-15): under 3e-7 in all, so 30 times over. Then t is positive and
//    finite: a hit.
// A hit sample is lit by every light when (one test per call, `lit_ok`,
// rtmi.cpp uniform_cam): every light has sd.y = -dir.y in (1e-6, 1e6], so its
// multiplier rcp(sd.y) is a positive number >= 0.99e-6; and
//   x = fl(fl(bias + fl(dy t + oy)) + ty) > 0.
// dy t = nroy (1 + e), |e| <= 2 eps (eps = 2^-23: rcp's ulp, the product's
// half ulp); nroy = -(oy + ty)(1 + e0), |e0| <= eps / 2; so fl(dy t + oy) is
// -ty within eps (|oy| / 2 + |ty| + 2 |nroy|), adding bias and ty rounds by
// at most eps (bias + |ty|) / 2 more, and the last rounding keeps the sign:
// x > 0 when bias > 2 eps (|oy| + |ty| + |nroy|) + eps bias / 2. The test asks
// for 16 eps (|oy| + |ty| + |nroy|), 8 times that, and bias >= 1e-30; then
// x >= 7/8 bias and ts = -x rcp(sd.y) is a negative normal number (>= 8e-37 in
// magnitude): the shadow ray misses the plane. Where the test fails (bias 0,
// a camera far from the plane, a light below or along the plane) no pixel is
// uniform-lit; uniform-sky does not depend on it.
struct UniformCam {
  int32_t on;      // 0: classify nothing (every lean pixel "mixed")
  int32_t m;       // samples per pixel side (grid_m)
  int32_t lit_ok;  // the call's condition for uniform-lit pixels
  float cam_a, cam_b, cam_c, cam_d, c4, c7, c10, st, of, nroy;
};
__host__ __device__ inline int uniform_class(const UniformCam& u, int x, int y) {
  if (!(fabsf(u.nroy) >= 1e-20f && fabsf(u.nroy) <= 1e20f)) return kUniMixed;
  float cx[2], cy[2];
  for (int k = 0; k < 2; ++k) {
    const float idx = k ? (float)(u.m - 1) : 0.0f;
    const float px = (float)x + fmaf(idx, u.st, u.of);
    cx[k] = (px - u.cam_b) * u.cam_a;
    const float py = (float)y + fmaf(idx, u.st, u.of);
    cy[k] = (u.cam_d - py) * u.cam_c;
  }
  bool pos = true, neg = true, fin = true;
  float amin = INFINITY;
  for (int i = 0; i < 2; ++i) {
    const float ay = fmaf(cx[i], u.c4, -u.c10);
    for (int j = 0; j < 2; ++j) {
      const float n = fmaf(cy[j], u.c7, ay);
      const float a = fabsf(n);
      pos = pos && n > 0.0f;
      neg = neg && n < 0.0f;
      fin = fin && a <= 1e10f;  // (false for a NaN)
      amin = a < amin ? a : amin;
    }
  }
  if (!fin || !(pos || neg)) return kUniMixed;
  if (pos != (u.nroy > 0.0f)) return kUniSky;
  if (!u.lit_ok) return kUniMixed;
  const double x2 = dmax((double)cx[0] * (double)cx[0], (double)cx[1] * (double)cx[1]);
  const double y2 = dmax((double)cy[0] * (double)cy[0], (double)cy[1] * (double)cy[1]);
  const double lo = (double)amin * (1.0 / sqrt(1.0 + x2 + y2)) * (1.0 - 1e-5);
  return lo > (double)1e-6f ? kUniLit : kUniMixed;
}

// ---- mesh pixels of gen1_loop (rt_fast.h gen1_batch): the inset box -------
//
// A shadow ray that leaves a hit on the mesh starts inside the mesh's box, and
// the gate (rt_fast.h mesh_gate: "a ray starting inside the box misses")
// answers false. The kernel proves that ahead of the gate with one test of the
// ray's origin against a box inset by a margin, the same for every light.
//
// lo, hi: the mesh object's float32 FObj.lo / FObj.hi. In float64,
//   m = 2^-12 max(|lo|_inf, |hi|_inf),
//   in_lo = nextafter(float(lo + m), +inf), in_hi = nextafter(float(hi - m), -inf),
// so a float strictly between in_lo and in_hi on an axis is more than m away
// from both of the box's planes there (the two roundings to float are
// covered by the step outwards of the true value).
//
// Lemma 1. ro strictly inside the inset box on all three axes, ni any floats
// with 1e-6 <= |ni| <= 1e20 (slab_ray's reciprocals, whatever v_rcp's last
// bit): mesh_gate is false. On an axis, with oi = fl(ro ni):
//   a = fl(lo ni - oi), b = fl(hi ni - oi)   (one rounding each: FMAs)
//   lo ni - oi = (lo - ro) ni + (ro ni - oi), |ro ni - oi| <= 2^-24 |ro| |ni|,
//   |(lo - ro) ni| > m |ni| >= 2^-12 |ro| |ni|   (|ro| < max(|lo|, |hi|)),
// so the exact lo ni - oi has the sign of (lo - ro) ni and the exact hi ni - oi
// the opposite one, both at least m |ni| (1 - 2^-12) >= 0.99e-31 in magnitude
// (m >= 1e-25): normal numbers, whose rounding keeps the sign, and at most
// 2e15 x 1e20 x 2: finite (|coordinates| <= 1e15). A product ro ni in the
// denormal range errs by at most 2^-149, far below m |ni|. So fminf(a, b) < 0
// on every axis, gmin < 0, and the gate's "gmin >= 0" fails.
//
// The call's condition (else the box is empty: lo = +inf, hi = -inf, no value
// is strictly between): every light's |v|_inf <= 1e6 (so |ni| >= 0.99e-6 on
// an unclamped component; a clamped one has |ni| = 1e20 within an ulp),
// m >= 1e-25, |coordinates| <= 1e15, in_lo < in_hi on all three axes.
struct InsetBox {
  float lo[3], hi[3];
};
// light_v: every light's FLight::v (3 floats each)
__host__ __device__ inline void inset_box(const float* lo, const float* hi, const float* light_v, int nl, InsetBox& b) {
  double amax = 0.0;
  for (int k = 0; k < 3; ++k) amax = dmax(amax, dmax(fabs((double)lo[k]), fabs((double)hi[k])));
  const double m = amax * (1.0 / 4096.0);
  bool ok = m >= 1e-25 && amax <= 1e15;  // (false for a NaN)
  for (int l = 0; l < 3 * nl; ++l) ok = ok && fabsf(light_v[l]) <= 1e6f;
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = nextafterf((float)((double)lo[k] + m), INFINITY);
    b.hi[k] = nextafterf((float)((double)hi[k] - m), -INFINITY);
    ok = ok && b.lo[k] < b.hi[k];
  }
  if (!ok)
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = INFINITY;
      b.hi[k] = -INFINITY;
    }
}
// (The kernel's test of a shadow origin against the box, compares alone, is
// rt_common.h inset_inside: the float32 kernels' unit does not include this
// file, whose float64 geometry is compiled without FMA contraction.)

}  // namespace bg
}  // namespace rtmi
