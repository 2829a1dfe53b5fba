// rt_query_rays.h — how the query kernels (rt_kernels_query.hip,
// rt_kernels_shade.hip) read ray i of a batch: one set of rules for what a
// ray is and when it is degenerate.
#pragma once
#include "rt_device.h"
#include "rt_query.h"

namespace rtmi {

__device__ __forceinline__ bool finite3(V3<double> v) {
  return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

// Ray i of the batch: (orig, dir, t_near) as given, or the camera ray
// through image position xy[i] — castPrimaryRay (renderer.nim:31-44) with
// k_render<double>'s operations — with t_near = +inf. Returns whether the ray
// is traced: not degenerate (a non-finite component, an all-zero direction,
// a NaN t_near; a pick: a non-finite position).
__device__ __forceinline__ bool query_ray(const RT_CONST RenderParams<double>& p, const QueryParams& q, long long i,
                                          V3<double>& o, V3<double>& d, double& tn) {
  using R = double;
  if (q.xy) {
    const R px = q.xy[2 * i], py = q.xy[2 * i + 1];
    const R cx = (Prec<R>::div(R(2) * px * p.aspect, R(p.width)) - p.aspect) * p.f;
    const R cy = (R(1) - Prec<R>::div(R(2) * py, R(p.height))) * p.f;
    const V3<R> dn = normalize_dir<R>(V3<R>{cx, cy, R(-1)});
    o = xform<R>(p.c2w, V3<R>{R(0), R(0), R(0)}, R(1));
    d = xform<R>(p.c2w, dn, R(0));
    tn = pinf<R>();
    return __builtin_isfinite(px) && __builtin_isfinite(py) && finite3(o) && finite3(d);
  }
  o = V3<R>{q.orig[3 * i], q.orig[3 * i + 1], q.orig[3 * i + 2]};
  d = V3<R>{q.dir[3 * i], q.dir[3 * i + 1], q.dir[3 * i + 2]};
  tn = q.tnear ? q.tnear[i] : pinf<R>();
  const bool zero = d.x == R(0) && d.y == R(0) && d.z == R(0);
  return finite3(o) && finite3(d) && !zero && !(tn != tn);
}

}  // namespace rtmi
