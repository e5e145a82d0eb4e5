// art_frame_math.hpp — per-collider decode, permeation loss terms and the baked-curve lookup,
// shared by the HIP kernels (art_kernels.hip) and the CPU backend (art_cpu.cpp) so both evaluate
// the reference's fp32 operation sequences from one source.
#pragma once

#include "art_device_fns.hpp"

#pragma clang fp contract(off)

namespace art {

// ------------------------------------------------------------------------------------------
// prep: decode colliders once per upload. Every value is computed exactly as the reference
// computes it per access (Center - Size, Radius * Radius, halfQuaternion decode, inverse), so
// hoisting is bit-identical.
// ------------------------------------------------------------------------------------------
// Broad-phase margins relative to the problem's scale (broad phase): the exact tests'
// rounding can report a blocking hit at most ~3 eps (boxes) or ~sqrt(20 eps) (sphere discriminant
// cancellation) times the scale away from the true shape; the factors below exceed those bounds
// by 10x or more.
#ifndef ART_CULL_MARGIN_SCALE
#define ART_CULL_MARGIN_SCALE 1.0f  // test hook: 0 disables the margins (tests/test_broadphase_gpu.py must fail)
#endif
constexpr float kCullBox = 1e-4f * ART_CULL_MARGIN_SCALE;
constexpr float kCullSphere = 4e-3f * ART_CULL_MARGIN_SCALE;
constexpr float kCullObb = 1e-3f * ART_CULL_MARGIN_SCALE;

ART_HD CullRec make_cull(float lx, float ly, float lz, float hx, float hy, float hz, float scale,
                                             float factor) {
  CullRec c;
  const bool fin = ufinite(lx) && ufinite(ly) && ufinite(lz) && ufinite(hx) && ufinite(hy) && ufinite(hz) &&
                   ufinite(scale);
  c.lox = fin ? lx : -INFINITY; c.loy = fin ? ly : -INFINITY; c.loz = fin ? lz : -INFINITY;
  c.hix = fin ? hx : INFINITY; c.hiy = fin ? hy : INFINITY; c.hiz = fin ? hz : INFINITY;
  c.fscale = fin ? factor * scale : 0.0f;
  c.factor = factor;
  return c;
}

// How far outside a sphere of radius r the reference's float test can report a hit, for a segment
// start within D of the centre (|oc| <= D): the sphere lemma of DESIGN.md §5 item 8. The reported
// point P satisfies |P - c|^2 <= r^2 + E, E = 13 eps |oc|^2 + 4 eps r^2 (the rounding of the
// discriminant), plus 16 eps (r + |oc|) for the rounding of oc, of the root and of the point. Two
// bounds follow: sqrt(r^2 + E) <= r + sqrt(E), tight only as r -> 0, which the margins have always
// used (kCullSphere's base factor times the scale), and sqrt(r^2 + E) <= r + E / (2 r), far smaller
// once r is not tiny against sqrt(eps) |oc|. The result is the smaller of the two, the second with a
// safety factor of kSlackSafety; r <= 0 or non-finite keeps the first.
#ifndef ART_SPHERE_SLACK_SCALE
#define ART_SPHERE_SLACK_SCALE 1.0f  // test hook: 0 disables the r-aware bound's slack (tests/test_sphere_slack_gpu.py must fail)
#endif
constexpr float kSlackEps = 5.9604645e-8f;  // 2^-24
constexpr float kSlackDisc = 13.0f, kSlackR2 = 4.0f, kSlackLin = 16.0f;  // E's and the linear term's constants, in eps
constexpr float kSlackRoot = 4e-3f;    // the square-root form: 4.5 x sqrt(13 eps) = 8.8e-4
constexpr float kSlackSafety = 2.0f;
ART_HD float sphere_report_slack(float r, float D) {
  const float root = kSlackRoot * D;
  if (!(r > 0.0f) || !ufinite(r)) return root;
  const float e = kSlackEps * (kSlackDisc * D * D + kSlackR2 * r * r);
  const float lin = (ART_SPHERE_SLACK_SCALE * kSlackSafety) * (e / (2.0f * r) + (kSlackLin * kSlackEps) * (r + D));
  return fminf(root, lin);
}

// Per-ray cap of a BVH node's margin (the capped node margin). A node that holds a
// sphere carries kCullSphere * (scale + om), the square-root form of the lemma above at the node's own
// scale; the r-aware form at the scene's smallest radius needs far less once r_min is not tiny. For a
// ray whose margin operand is om, every collider centre lies within D = s_root + om of the ray's start,
// s_root = node_abs_sum of the BVH root's stored box (it bounds |c|_1 + r and |c|_1 + |h|_1 of every
// collider). The cap is the larger of
//   kNodeCapSlack * sphere_report_slack(r_min, D)   what a sphere of any radius in [r_min, D] needs, and
//   kNodeCapGuard * kF * D                          at least every box's (OBB's) own margin kF * (scale + om),
// kF = kCullObb with OBBs in the scene, else kCullBox, so that a node without a sphere never sees the cap
// bind: m = min(fma(factor, om, fscale), cap) is then fma's value bit for bit. kNodeCapSlack (s): a reported
// point lies within half of the helper's value (its safety factor) of the sphere, and the BVH argument wants
// it 3/4 of the margin inside the widened box, so s >= 2/3 does; s = 1 leaves a factor 1.5 on the proven
// bound, 3.7 on the worst hit measured (tests/test_sphere_slack_cpu.py), and measured faster than s = 2
// (profiles/node_margin_cap_ab.txt).
// kNodeCapGuard: an OBB's scale is |c|_1 + 1.001 |h|_1 while its world box may sum to |c|_1 + 1.00013 |h|_1,
// and the two sums round in different orders; 1 % covers both.
// `reach` (the logging cast, log_margin_om): the part of the operand that pays for the echo replay's
// reach keeps its full factor, cap + kCullSphere * reach, with om the operand's base part.
// No cap (+infinity, min keeps fma's value): r_min zero, negative, NaN or infinite (no sphere, or a
// radius the r-aware form cannot use), or a non-finite s_root, om or reach.
#ifndef ART_NODE_CAP_SLACK_SCALE
#define ART_NODE_CAP_SLACK_SCALE 1.0f  // test hook: 0 leaves the cap its floor alone (tests/test_node_margin_gpu.py must fail)
#endif
constexpr float kNodeCapSlack = 1.0f * ART_NODE_CAP_SLACK_SCALE, kNodeCapGuard = 1.01f;
ART_HD float node_abs_sum(float lox, float loy, float loz, float hix, float hiy, float hiz) {
  return fmaxf(fabsf(lox), fabsf(hix)) + fmaxf(fabsf(loy), fabsf(hiy)) + fmaxf(fabsf(loz), fabsf(hiz));
}
// The helper in two steps, so that a kernel pays no division per ray: the r-aware form of sphere_report_slack is a
// quadratic in D whose coefficients depend on r_min alone (the host keeps them beside DevScene::r_min), and the
// per-ray step is that polynomial, the square-root form, the floor and the reach term (about 15 VALU).
ART_HD NodeCapCoef node_cap_coef(float r_min) {
  NodeCapCoef c;
  c.a2 = c.a1 = c.a0 = c.on = 0.0f;
  if (!(r_min > 0.0f) || !ufinite(r_min)) return c;
  const float k = (ART_SPHERE_SLACK_SCALE * kSlackSafety * kNodeCapSlack) * kSlackEps;
  c.a2 = k * kSlackDisc / (2.0f * r_min);                    // E / (2 r)'s D^2 part
  c.a1 = k * kSlackLin;                                      // 16 eps D
  c.a0 = k * (0.5f * kSlackR2 + kSlackLin) * r_min;          // E / (2 r)'s r part and 16 eps r
  c.on = 1.0f;
  return c;
}
ART_HD float node_cap_eval(const NodeCapCoef& c, float D, float kf, float reach) {
  if (!(c.on > 0.0f) || !ufinite(D) || !ufinite(reach)) return INFINITY;
  const float lin = (c.a2 * D + c.a1) * D + c.a0;
  return fmaxf(fminf((kNodeCapSlack * kSlackRoot) * D, lin), (kNodeCapGuard * kf) * D) + kCullSphere * reach;
}
ART_HD float node_margin_cap(float r_min, float s_root, float om, bool has_obb, float reach) {
  return node_cap_eval(node_cap_coef(r_min), s_root + om, has_obb ? kCullObb : kCullBox, reach);
}
inline void set_r_min(DevScene& sc, float r_min) {
  sc.r_min = r_min;
  sc.cap = node_cap_coef(r_min);
}

// Per-collider decode (shared by the full prep and the resident store's scatter): the hot/cold
// records at in-kind index i and the broad-phase bounds at global index gi.
ART_HD void prep_sphere(const art_sphere& s, int i, int gi, SphereRec* __restrict__ osph,
                                            SphereCold* __restrict__ osphc, CullRec* __restrict__ cull) {
  SphereRec r;
  r.cx = f16tof32(s.center.x); r.cy = f16tof32(s.center.y); r.cz = f16tof32(s.center.z);
  float rad = f16tof32(s.radius);
  r.r2 = rad * rad;
  r.tid = s.audio_target_id;
  r.pad0 = r.pad1 = r.pad2 = 0;
  SphereCold c;
  c.density = f16tof32(s.material.density);
  c.absorption = f16tof32(s.material.absorption);
  c.echo = f16tof32(s.material.echo);
  c.pad = 0.0f;
  osph[i] = r;
  osphc[i] = c;
  const float ra = fabsf(rad);
  cull[gi] = make_cull(r.cx - ra, r.cy - ra, r.cz - ra, r.cx + ra, r.cy + ra, r.cz + ra,
                       fabsf(r.cx) + fabsf(r.cy) + fabsf(r.cz) + ra, kCullSphere);
}

ART_HD void prep_aabb(const art_aabb& a, int i, int gi, AabbRec* __restrict__ oaabb,
                                          AabbCold* __restrict__ oaabbc, CullRec* __restrict__ cull) {
  AabbCold c;
  c.cx = f16tof32(a.center.x); c.cy = f16tof32(a.center.y); c.cz = f16tof32(a.center.z);
  c.hx = f16tof32(a.size.x); c.hy = f16tof32(a.size.y); c.hz = f16tof32(a.size.z);
  c.density = f16tof32(a.material.density);
  c.absorption = f16tof32(a.material.absorption);
  c.echo = f16tof32(a.material.echo);
  c.pad0 = c.pad1 = c.pad2 = 0.0f;
  AabbRec r;
  r.mnx = c.cx - c.hx; r.mny = c.cy - c.hy; r.mnz = c.cz - c.hz;
  r.mxx = c.cx + c.hx; r.mxy = c.cy + c.hy; r.mxz = c.cz + c.hz;
  r.tid = a.audio_target_id;
  r.pad = 0.0f;
  oaabb[i] = r;
  oaabbc[i] = c;
  cull[gi] = make_cull(fminf(r.mnx, r.mxx), fminf(r.mny, r.mxy), fminf(r.mnz, r.mxz), fmaxf(r.mnx, r.mxx),
                       fmaxf(r.mny, r.mxy), fmaxf(r.mnz, r.mxz),
                       fabsf(c.cx) + fabsf(c.cy) + fabsf(c.cz) + fabsf(c.hx) + fabsf(c.hy) + fabsf(c.hz), kCullBox);
}

ART_HD void prep_obb(const art_obb& b, int i, int gi, ObbRec* __restrict__ oobb,
                                         ObbCold* __restrict__ oobbc, CullRec* __restrict__ cull) {
  ObbRec r;
  ObbCold c;
  r.cx = f16tof32(b.center.x); r.cy = f16tof32(b.center.y); r.cz = f16tof32(b.center.z);
  c.hx = f16tof32(b.size.x); c.hy = f16tof32(b.size.y); c.hz = f16tof32(b.size.z);
  r.lmnx = 0.0f - c.hx; r.lmny = 0.0f - c.hy; r.lmnz = 0.0f - c.hz;
  r.lmxx = 0.0f + c.hx; r.lmxy = 0.0f + c.hy; r.lmxz = 0.0f + c.hz;
  r.pad0 = r.pad1 = 0.0f;
  quat q = half_quaternion_value(b.rot_x, b.rot_y, b.rot_z);
  quat qi = qinverse(q);
  r.qx = q.x; r.qy = q.y; r.qz = q.z; r.qw = q.w;
  c.iqx = qi.x; c.iqy = qi.y; c.iqz = qi.z; c.iqw = qi.w;
  r.tid = b.audio_target_id;
  c.density = f16tof32(b.material.density);
  c.absorption = f16tof32(b.material.absorption);
  c.echo = f16tof32(b.material.echo);
  c.pad0 = c.pad1 = 0.0f;
  oobb[i] = r;
  oobbc[i] = c;
  // World bounds of the rotated box (round 4; round 3 used the cube of half-width |h|_1, up to 8x the
  // volume). The tests map P - c to the local frame by the stored rotation R (ShootRayCast
  // :314-320, permeation loss :294-300) or by its inverse R^T (permeation first hit :172-179), so a
  // point reported inside the local box [-h, h] lies within half_i = max(sum_j |R_ji| h_j,
  // sum_j |R_ij| h_j) of c on world axis i. Column i of R is qmul(q, e_i); the relative and absolute
  // slack covers the rounding of these entries (each within ~10 eps), the margins the rest
  // (the margin scale keeps |h|_1).
  const float h1 = fabsf(c.hx) + fabsf(c.hy) + fabsf(c.hz);
  const float rho = h1 * 1.001f;
  const bool qok = ufinite(q.x) && ufinite(q.y) && ufinite(q.z) && ufinite(q.w);
  const vec3 ax = qmul(q, mk3(1.0f, 0.0f, 0.0f)), ay = qmul(q, mk3(0.0f, 1.0f, 0.0f)), az = qmul(q, mk3(0.0f, 0.0f, 1.0f));
  const vec3 ha = abs3(mk3(c.hx, c.hy, c.hz));
  const vec3 cx = abs3(ax), cy = abs3(ay), cz = abs3(az);  // |columns| of R
  const float slack = 1e-5f * h1;
  const float wx = fmaxf(cx.x * ha.x + cx.y * ha.y + cx.z * ha.z, cx.x * ha.x + cy.x * ha.y + cz.x * ha.z);
  const float wy = fmaxf(cy.x * ha.x + cy.y * ha.y + cy.z * ha.z, cx.y * ha.x + cy.y * ha.y + cz.y * ha.z);
  const float wz = fmaxf(cz.x * ha.x + cz.y * ha.y + cz.z * ha.z, cx.z * ha.x + cy.z * ha.y + cz.z * ha.z);
  const float bx = fminf(wx * 1.0001f + slack, rho), by = fminf(wy * 1.0001f + slack, rho), bz = fminf(wz * 1.0001f + slack, rho);
  cull[gi] = make_cull(r.cx - bx, r.cy - by, r.cz - bz, r.cx + bx, r.cy + by, r.cz + bz,
                       qok ? fabsf(r.cx) + fabsf(r.cy) + fabsf(r.cz) + rho : INFINITY, kCullObb);
}


// ------------------------------------------------------------------------------------------
// Permeation loss terms (AudioPermeationJobBatched.cs:265-328)
// ------------------------------------------------------------------------------------------
ART_HD float perm_term_sphere(const Seg& s, const SphereRec& c, float density) {
  // RayIntersectsSpherePermeation :303-328
  vec3 oc = s.o - mk3(c.cx, c.cy, c.cz);
  float b = dot(oc, s.d);
  float cc = dot(oc, oc) - c.r2;
  float disc = b * b - cc;
  if (disc < 0.0f) return 0.0f;
  float sq = sqrtf(disc);
  float tEnter = -b - sq, tExit = -b + sq;
  if (tExit < 0.0f) return 0.0f;
  float enter = umax(tEnter, 0.0f);
  return umax(0.0f, tExit - enter) * density;
}
ART_HD float perm_term_slab(float ox, float oy, float oz, float ix, float iy, float iz, float mnx,
                                                float mny, float mnz, float mxx, float mxy, float mxz, float density) {
  // RayIntersectsAABBPermeation :265-288
  float tEnter, tExit;
  if (!slab<false>(ox, oy, oz, ix, iy, iz, mnx, mny, mnz, mxx, mxy, mxz, tEnter, tExit)) return 0.0f;
  float enter = umax(tEnter, 0.0f);
  return umax(0.0f, tExit - enter) * density;
}


// NativeSampledAnimationCurve.EvaluateWithBurst (DataTypes/NativeSampledAnimationCurve.cs:81-89)
ART_HD float curve_eval(const float* baked, int n, float length, float time) {
  float percent = time / length;
  float cp = umax(0.0f, umin((float)(n - 1), percent * (float)(n - 1)));
  int fi = (int)floorf(cp), ci = (int)ceilf(cp);
  return ulerp(baked[fi], baked[ci], cp - (float)fi);
}


}  // namespace art
