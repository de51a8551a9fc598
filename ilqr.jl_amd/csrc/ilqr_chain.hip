// MI355X (gfx950) kernels + C ABI of the RBD problem family (ILQR_PROBLEM_CHAIN):
// a fixed-base serial chain of revolute joints described by a URDF — the
// reference's RigidBodyDynamics.jl example (test/RBD_2_link_example/
// RBD_helper_functions.jl:48-116 on test/urdf/2Dof_arm.urdf; BASELINE.json
// config 5) with a fixed base.
//
// What replaces what:
//  * dynamicsf (:48-79): RK4 of v̇ = M(q) \ (τ − dynamics_bias(q, v)), q̇ = v. The
//    device functor is Featherstone's recursive Newton-Euler (the published
//    algorithm behind RBD.jl's dynamics_bias) for the bias, and M's columns from the
//    same recursion with unit accelerations; everything templated on the scalar
//    (float / double / DualT<N, ·>).
//  * linearize_dynamics (src/backward_pass.jl:25-40, ForwardDiff): forward-mode dual
//    numbers (ILQR_LINEARIZE_DUAL, exact like the reference) or central finite
//    differences (ILQR_LINEARIZE_CENTRAL_FD, what BASELINE config 5 names), one lane
//    per (trajectory, step, direction); on the tiles path also ILQR_LINEARIZE_ANALYTIC, the
//    duals' Jacobians from the tangent of the Newton-Euler pass at fixed q̈
//    (chain_linearize_analytic_kernel).
//  * immediate_cost / final_cost (:85-116) on the joint rows: Σ qwᵢ(θ*ᵢ−θᵢ)² + Σ rwₖuₖ²
//    and Σ qfwᵢ(θ*ᵢ−θᵢ)²; their derivatives are the exact constants.
//  * backward_pass / forward_pass / fit: the Riccati recursion (four trajectories per
//    wave on the 4-block f64 MFMA for 2-joint chains, lane per trajectory otherwise)
//    and the RK4 rollout + α-halving line search (a 16-lane group per trajectory,
//    component-parallel Newton-Euler for chains of ≤ 3 joints), in the handle's dtype
//    (fp32 or fp64). Four to seven joints, every joint driven (the 6-DoF arm, a
//    7-DoF manipulator; fp64): the linearisation and the costs written as tiles for the
//    tiles recursion (ilqr_tiles.hip) and a 32-lane forward group per trajectory —
//    "Chains on the tiles path" below.
//  * cost_functions.jl's simple_final_cost / simple_immediate_cost (src/cost_functions.jl:
//    5-54) in place of the joint-space costs: on 2-joint chains the point's coordinates as
//    a polynomial sampled at the call (ChainTask, ilqr_chain_set_simple_costs, closed-form
//    dynamics only); on the tiles path the kinematics composed on the device at every
//    evaluation, analytic derivatives as the terminal tiles and the task cost inside the
//    32-lane forward group (ChainTaskK, ilqr_chain_set_task_costs,
//    ilqr_chain_final_cost_quadratize; fp64). ilqr_chain_set_simple_costs keeps refusing
//    more than two joints, and an fp32 handle of more than two joints answers dynamics only.
//  * a goal per trajectory on the tiles path (ilqr_chain_set_joint_targets: θ*,
//    ilqr_chain_set_task_targets: final_target): the handle's copy of the rows, read by the
//    ChainGoalRows instantiations of the cost tiles, the task quadratization and the forward
//    kernels; a handle without rows launches the instantiations it always did.
// Layout as the other families (include/ilqr.h): x (B, T+1, nx), u/d (B, T, nu),
// K (B, T, nu, nx), trajectory slowest, nx = 2·n_joints.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/ilqr.h"
#include "ilqr_fit.h"
#include "ilqr_internal.h"
#include "ilqr_device.h"
#include "ilqr_math.h"
#include "ilqr_fwd_group.h"

namespace ilqr {
namespace {

// ---------------------------------------------------------------------------
// scalar helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ void vsincos(float x, float& s, float& c) { fast_sincosf(x, s, c); }
__device__ __forceinline__ void vsincos(double x, double& s, double& c) { fast_sincos(x, s, c); }

// Forward-mode dual number over value type V (ForwardDiff.Dual restated).
template <int N, class V>
struct DualT {
  V v;
  V d[N];
  DualT() = default;
  __device__ __forceinline__ DualT(V c) : v(c) {
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = V(0);
  }
};
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator+(const DualT<N, V>& a, const DualT<N, V>& b) {
  DualT<N, V> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator-(const DualT<N, V>& a, const DualT<N, V>& b) {
  DualT<N, V> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator-(const DualT<N, V>& a) {
  DualT<N, V> r;
  r.v = -a.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = -a.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator*(const DualT<N, V>& a, const DualT<N, V>& b) {
  DualT<N, V> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator*(V a, const DualT<N, V>& b) {
  DualT<N, V> r;
  r.v = a * b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a * b.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator*(const DualT<N, V>& b, V a) { return a * b; }
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator+(V a, const DualT<N, V>& b) {
  DualT<N, V> r = b;
  r.v = a + b.v;
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator-(V a, const DualT<N, V>& b) {
  DualT<N, V> r = -b;
  r.v = a - b.v;
  return r;
}
template <int N, class V>
__device__ __forceinline__ DualT<N, V> operator/(V a, const DualT<N, V>& b) {
  DualT<N, V> r;  // (a/b)' = −(a/b) b'/b
  r.v = a / b.v;
  const V k = -r.v / b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = k * b.d[i];
  return r;
}
template <int N, class V>
__device__ __forceinline__ void scs(const DualT<N, V>& a, DualT<N, V>& s, DualT<N, V>& c) {
  V sv, cv;
  vsincos(a.v, sv, cv);
  s.v = sv;
  c.v = cv;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    s.d[i] = cv * a.d[i];
    c.d[i] = -sv * a.d[i];
  }
}
__device__ __forceinline__ void scs(float a, float& s, float& c) { vsincos(a, s, c); }
__device__ __forceinline__ void scs(double a, double& s, double& c) { vsincos(a, s, c); }
// 1/x of the mass-matrix pivots: fp32 by v_rcp_f32 and one Newton step (within an
// ulp of the IEEE quotient; the IEEE division's scale/fixup sequence sat on the
// rollout's dependent chain), fp64 and duals by division
__device__ __forceinline__ float crecip(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ double crecip(double x) { return 1.0 / x; }
template <int N, class V>
__device__ __forceinline__ DualT<N, V> crecip(const DualT<N, V>& x) { return V(1) / x; }

// a pair of fp32 evaluations carried together (packed v_pk_* arithmetic)
typedef float F2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void scs(F2 a, F2& s, F2& c) {
  float s0, c0, s1, c1;
  vsincos(a.x, s0, c0);
  vsincos(a.y, s1, c1);
  s = F2{s0, s1};
  c = F2{c0, c1};
}
__device__ __forceinline__ F2 crecip(F2 x) {
  const F2 r = F2{__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)};
  return (F2(1.0f) - x * r) * r + r;
}

template <class S> struct ValueOf { using type = S; };
template <int N, class V> struct ValueOf<DualT<N, V>> { using type = V; };

// ---------------------------------------------------------------------------
// Chain constants in the kernel's value type (converted from ilqr_chain on the host)
// ---------------------------------------------------------------------------
template <class V, int NJ>
struct ChainK {
  V R0[NJ][9];  // joint frame → parent body frame, row-major
  V R0x[NJ][9];  // R0·[a]×   } so that R0·Rot(a, q) = c·R0 + s·R0x + (1−c)·R0aa
  V R0aa[NJ][9]; // R0·a·aᵀ   } (Rodrigues expanded over the constant factors)
  V p[NJ][3];   // joint origin in the parent body frame
  V ax[NJ][3];  // unit axis (joint = child frame)
  V m[NJ];
  V mc[NJ][3];  // m · COM
  V Io[NJ][9];  // rotational inertia about the body origin
  V g[3];       // gravity
  V dt;
  V tgt[NJ], qw[NJ], rw[NJ], qfw[NJ];  // joint-space cost (RBD_helper_functions.jl:85-116)
};

template <class S>
__device__ __forceinline__ void cross3(const S (&a)[3], const S (&b)[3], S (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// a × b with a constant
template <class S, class V>
__device__ __forceinline__ void crossc(const V (&a)[3], const S (&b)[3], S (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// The joint transform R_i = R0_i Rot(a_i, q_i) (joint frame → parent body frame),
// built once per evaluation from (cos q, sin q): 9 × 3 ops, after which each of the
// recursion's 6 coordinate changes per joint is a 3×3 product (9 ops) instead of an
// in-place Rodrigues rotation (≈28). v7; the v6 form rotated every vector.
template <class S, class V, int NJ>
__device__ __forceinline__ void joint_rot(const ChainK<V, NJ>& P, int i, const S& c, const S& s,
                                          S (&R)[9]) {
  const S omc = V(1) - c;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = c * P.R0[i][k] + s * P.R0x[i][k] + omc * P.R0aa[i][k];
}
// parent → child coordinates: w_c = R_iᵀ w_p
template <class S>
__device__ __forceinline__ void to_child(const S (&R)[9], const S (&w)[3], S (&o)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = R[r] * w[0] + R[3 + r] * w[1] + R[6 + r] * w[2];
}
// child → parent: w_p = R_i w_c
template <class S>
__device__ __forceinline__ void to_parent(const S (&R)[9], const S (&w)[3], S (&o)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = R[3 * r] * w[0] + R[3 * r + 1] * w[1] + R[3 * r + 2] * w[2];
}

// Recursive Newton-Euler: τ = M(q) q̈ + [VEL] C(q, q̇)q̇ + [GRAV] g(q).
// qd is read only when VEL; qdd[i] is the joint acceleration.
// gs scales gravity (the lane-split forward runs the bias and the mass-matrix
// columns as one uniform pass with per-lane q̇, q̈ and gravity; 1 elsewhere, folded)
template <bool VEL, bool GRAV, int NJ, class S, class V>
__device__ __forceinline__ void rnea(const ChainK<V, NJ>& P, const S (&c)[NJ], const S (&s)[NJ],
                                     const S (&qd)[NJ], const S (&qdd)[NJ], S (&tau)[NJ],
                                     V gs = V(1)) {
  S w[3], v[3], al[3], ac[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    w[r] = S(V(0));
    v[r] = S(V(0));
    al[r] = S(V(0));
    ac[r] = S(GRAV ? -P.g[r] * gs : V(0));  // fictitious base acceleration −g
  }
  // joint transforms as 3×3 products of the per-evaluation R_i (in-place Rodrigues
  // rotations measured slower once the linearisation ran one direction per lane,
  // DESIGN.md §4; tools/ablation/restore_alternates.patch)
  S fn[NJ][3], ff[NJ][3], R[NJ][9];
#pragma unroll
  for (int i = 0; i < NJ; ++i) joint_rot(P, i, c[i], s[i], R[i]);
  auto tc = [&](int i, const S (&w)[3], S (&o)[3]) { to_child(R[i], w, o); };
  auto tp = [&](int i, const S (&w)[3], S (&o)[3]) { to_parent(R[i], w, o); };
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    S t[3], u3[3];
    // spatial motion transform to body i: ω_i = X ω, v_i = X (v − p × ω) (same for accel)
    S wi[3], vi[3], ali[3], aci[3];
    tc(i, w, wi);
    crossc(P.p[i], w, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) u3[r] = v[r] - t[r];
    tc(i, u3, vi);
    tc(i, al, ali);
    crossc(P.p[i], al, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) u3[r] = ac[r] - t[r];
    tc(i, u3, aci);
    if constexpr (VEL) {
      S sq[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) sq[r] = P.ax[i][r] * qd[i];  // S q̇
#pragma unroll
      for (int r = 0; r < 3; ++r) wi[r] = wi[r] + sq[r];
      cross3(wi, sq, t);  // (v ×m S q̇): angular part ω × Sq̇, linear part v × Sq̇
#pragma unroll
      for (int r = 0; r < 3; ++r) ali[r] = ali[r] + t[r];
      cross3(vi, sq, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) aci[r] = aci[r] + t[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) ali[r] = ali[r] + P.ax[i][r] * qdd[i];
    // f = I a + v ×f (I v),  I·(α, a) = (Io α + mc × a, m a − mc × α)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      fn[i][r] = P.Io[i][3 * r] * ali[0] + P.Io[i][3 * r + 1] * ali[1] + P.Io[i][3 * r + 2] * ali[2];
    crossc(P.mc[i], aci, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) fn[i][r] = fn[i][r] + t[r];
    crossc(P.mc[i], ali, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) ff[i][r] = P.m[i] * aci[r] - t[r];
    if constexpr (VEL) {
      S hn[3], hf[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        hn[r] = P.Io[i][3 * r] * wi[0] + P.Io[i][3 * r + 1] * wi[1] + P.Io[i][3 * r + 2] * wi[2];
      crossc(P.mc[i], vi, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) hn[r] = hn[r] + t[r];
      crossc(P.mc[i], wi, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) hf[r] = P.m[i] * vi[r] - t[r];
      cross3(wi, hn, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) fn[i][r] = fn[i][r] + t[r];
      cross3(vi, hf, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) fn[i][r] = fn[i][r] + t[r];
      cross3(wi, hf, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) ff[i][r] = ff[i][r] + t[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      w[r] = wi[r];
      v[r] = vi[r];
      al[r] = ali[r];
      ac[r] = aci[r];
    }
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    tau[i] = P.ax[i][0] * fn[i][0] + P.ax[i][1] * fn[i][1] + P.ax[i][2] * fn[i][2];
    if (i > 0) {
      S pf[3], pn[3], t[3];
      tp(i, ff[i], pf);
      tp(i, fn[i], pn);
      crossc(P.p[i], pf, t);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        fn[i - 1][r] = fn[i - 1][r] + (pn[r] + t[r]);
        ff[i - 1][r] = ff[i - 1][r] + pf[r];
      }
    }
  }
}

// [q̇; v̇] with v̇ = M \ (τ − bias)  (RBD_helper_functions.jl:61-66).
// nu = NJ drives every joint; nu = 1 drives joint 1 only.
template <int NJ, int NU, class S, class V>
__device__ __forceinline__ void chain_xdot(const ChainK<V, NJ>& P, const S (&x)[2 * NJ],
                                           const S (&u)[NU], S (&xd)[2 * NJ]) {
  S c[NJ], s[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) scs(x[i], s[i], c[i]);
  S zero[NJ], qd[NJ], b[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    zero[i] = S(V(0));
    qd[i] = x[NJ + i];
  }
  rnea<true, true>(P, c, s, qd, zero, b);  // dynamics_bias
  S M[NJ][NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {  // mass_matrix, column k = RNEA(q, 0, e_k)
    S e[NJ], col[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) e[j] = S(V(j == k ? 1 : 0));
    rnea<false, false>(P, c, s, zero, e, col);
#pragma unroll
    for (int i = 0; i < NJ; ++i) M[i][k] = col[i];
  }
  S r[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) r[i] = (i < NU ? u[i < NU ? i : 0] : S(V(0))) - b[i];
  // Gaussian elimination (M is SPD: no pivoting)
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const S inv = crecip(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < NJ; ++i) {
      const S l = M[i][k] * inv;
#pragma unroll
      for (int j = k + 1; j < NJ; ++j) M[i][j] = M[i][j] - l * M[k][j];
      r[i] = r[i] - l * r[k];
    }
  }
  S qdd[NJ];
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    S acc = r[i];
#pragma unroll
    for (int j = i + 1; j < NJ; ++j) acc = acc - M[i][j] * qdd[j];
    qdd[i] = acc * crecip(M[i][i]);
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    xd[i] = x[NJ + i];
    xd[NJ + i] = qdd[i];
  }
}

// ---------------------------------------------------------------------------
// Component-parallel Newton-Euler (v7 forward): a 16-lane group per trajectory,
// lane 4·role + c. The role picks the pass (0: bias with q̇ and gravity, k+1: M's
// column k), c ∈ {0,1,2} holds component c of every 3-vector (lane 3 of each quad
// computes a copy of component 0 and is never read). Cross products, rotations and
// dot products reach the other components of the same quad through DPP quad
// permutations, so each lane issues about a third of the scalar pass's arithmetic;
// the arithmetic per component is the scalar pass's, in the same order up to the
// association of three-term sums.
// ---------------------------------------------------------------------------
// bound_ctrl set: every source lane of a quad_perm / row_newbcast is valid, so it
// changes nothing but lets the compiler fold the move into a VOP2 consumer
// (v_mul_f32_dpp, v_add_f32_dpp: forward 1,733 → 1,653 instructions)
template <int CTRL, class V>
__device__ __forceinline__ V qperm(V x) {  // quad_perm DPP move
  if constexpr (sizeof(V) == 4) {
    return __builtin_bit_cast(V, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
  } else {
    const u2v p = __builtin_bit_cast(u2v, x);
    const u2v q = {(unsigned)__builtin_amdgcn_mov_dpp((int)p.x, CTRL, 0xF, 0xF, true),
                   (unsigned)__builtin_amdgcn_mov_dpp((int)p.y, CTRL, 0xF, 0xF, true)};
    return __builtin_bit_cast(V, q);
  }
}
constexpr int QP_B0 = 0x00, QP_B1 = 0x55, QP_B2 = 0xAA;  // broadcast component k
constexpr int QP_R1 = 0xC9, QP_R2 = 0xD2;                // component c+1 / c+2 (mod 3)
constexpr int QP_ROWBC = 0x150;                         // row_newbcast:n = 0x150 + n
// lane 4·role (component 0 of that pass) of the row, broadcast to the row
template <class V> __device__ __forceinline__ V rowbc_role(V x, int role) {
  return role == 1 ? qperm<QP_ROWBC + 4>(x) : role == 2 ? qperm<QP_ROWBC + 8>(x) : qperm<QP_ROWBC + 12>(x);
}
template <class V> __device__ __forceinline__ V bc0(V x) { return qperm<QP_B0>(x); }
template <class V> __device__ __forceinline__ V bc1(V x) { return qperm<QP_B1>(x); }
template <class V> __device__ __forceinline__ V bc2(V x) { return qperm<QP_B2>(x); }
template <class V> __device__ __forceinline__ V r1(V x) { return qperm<QP_R1>(x); }
template <class V> __device__ __forceinline__ V r2(V x) { return qperm<QP_R2>(x); }
// (a × b)_c = a_{c+1} b_{c+2} − a_{c+2} b_{c+1}
template <class V> __device__ __forceinline__ V cv_cross(V a, V b) { return r1(a) * r2(b) - r2(a) * r1(b); }
// constant a: the lane holds a1 = a_{c+1}, a2 = a_{c+2}
template <class V> __device__ __forceinline__ V cv_crossc(V a1, V a2, V b) { return a1 * r2(b) - a2 * r1(b); }
// Σ_k m_k w_k with m_k the lane's row (m[c][k]) or column entries
template <class V> __device__ __forceinline__ V cv_mat(V m0, V m1, V m2, V w) {
  return m0 * bc0(w) + m1 * bc1(w) + m2 * bc2(w);
}

template <bool VEL, bool GRAV, int NJ, class V>
__device__ __forceinline__ void rnea_cv(const ChainK<V, NJ>& P, const V (&c)[NJ], const V (&s)[NJ],
                                        const V (&qd)[NJ], const V (&qdd)[NJ], V (&tau)[NJ], V gs,
                                        int cmp) {
  const int c0 = cmp < 3 ? cmp : 0;
  const int c1 = c0 == 2 ? 0 : c0 + 1, c2 = c0 == 0 ? 2 : c0 - 1;
  V w = V(0), v = V(0), al = V(0), ac = GRAV ? -P.g[c0] * gs : V(0);
  V fn[NJ], ff[NJ], Rr[NJ][3], Rc[NJ][3];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {  // row c and column c of R_i = R0 Rot(a, q)
    const V omc = V(1) - c[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Rr[i][k] = c[i] * P.R0[i][3 * c0 + k] + s[i] * P.R0x[i][3 * c0 + k] + omc * P.R0aa[i][3 * c0 + k];
      Rc[i][k] = c[i] * P.R0[i][3 * k + c0] + s[i] * P.R0x[i][3 * k + c0] + omc * P.R0aa[i][3 * k + c0];
    }
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const V p1 = P.p[i][c1], p2 = P.p[i][c2], mc1 = P.mc[i][c1], mc2 = P.mc[i][c2];
    const V axc = P.ax[i][c0];
    // to_child: w_c = Σ_k R[k][c] w_k
    V wi = cv_mat(Rc[i][0], Rc[i][1], Rc[i][2], w);
    V vi = cv_mat(Rc[i][0], Rc[i][1], Rc[i][2], v - cv_crossc(p1, p2, w));
    V ali = cv_mat(Rc[i][0], Rc[i][1], Rc[i][2], al);
    V aci = cv_mat(Rc[i][0], Rc[i][1], Rc[i][2], ac - cv_crossc(p1, p2, al));
    if constexpr (VEL) {
      const V sq = axc * qd[i];
      wi = wi + sq;
      ali = ali + cv_cross(wi, sq);
      aci = aci + cv_cross(vi, sq);
    }
    ali = ali + axc * qdd[i];
    fn[i] = cv_mat(P.Io[i][3 * c0], P.Io[i][3 * c0 + 1], P.Io[i][3 * c0 + 2], ali) + cv_crossc(mc1, mc2, aci);
    ff[i] = P.m[i] * aci - cv_crossc(mc1, mc2, ali);
    if constexpr (VEL) {
      const V hn = cv_mat(P.Io[i][3 * c0], P.Io[i][3 * c0 + 1], P.Io[i][3 * c0 + 2], wi) + cv_crossc(mc1, mc2, vi);
      const V hf = P.m[i] * vi - cv_crossc(mc1, mc2, wi);
      fn[i] = fn[i] + cv_cross(wi, hn);
      fn[i] = fn[i] + cv_cross(vi, hf);
      ff[i] = ff[i] + cv_cross(wi, hf);
    }
    w = wi;
    v = vi;
    al = ali;
    ac = aci;
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    const V pr = P.ax[i][c0] * fn[i];  // S_iᵀ f_i over the three components
    tau[i] = (bc0(pr) + bc1(pr)) + bc2(pr);
    if (i > 0) {
      const V pf = cv_mat(Rr[i][0], Rr[i][1], Rr[i][2], ff[i]);  // to_parent: Σ_k R[c][k] f_k
      const V pn = cv_mat(Rr[i][0], Rr[i][1], Rr[i][2], fn[i]);
      fn[i - 1] = fn[i - 1] + (pn + cv_crossc(P.p[i][c1], P.p[i][c2], pf));
      ff[i - 1] = ff[i - 1] + pf;
    }
  }
}

// chain_xdot over a 16-lane group: role = pass, c = component (see rnea_cv); every
// lane of the group ends with the same [q̇; v̇]
template <int NJ, int NU, class V>
__device__ __forceinline__ void chain_xdot_cv(const ChainK<V, NJ>& P, const V (&x)[2 * NJ],
                                              const V (&u)[NU], V (&xd)[2 * NJ]) {
  static_assert(NJ + 1 <= 4, "one role per pass in a group of 16");
  // lane c of a quad evaluates joint min(c, NJ − 1) and the quad reads joint i from its
  // lane i (bc0/bc1/bc2 below): only joints 0..2 have a broadcast
  static_assert(NJ <= 3, "one sin/cos per lane: a quad holds at most three joints");
  const int l16 = threadIdx.x & 15;
  const int role = l16 >> 2, cmp = l16 & 3;
  V c[NJ], s[NJ], qd[NJ], qdd[NJ], tau[NJ];
  // one sin/cos per lane: lane c of each quad evaluates joint min(c, NJ − 1), and the
  // quad reads joint i's pair from its lane i by DPP quad broadcast (the same bits as
  // evaluating every joint in every lane, at one polynomial pair per lane)
  V ang = x[0];
#pragma unroll
  for (int i = 1; i < NJ; ++i)
    if (cmp >= i) ang = x[i];
  V so, co;
  scs(ang, so, co);
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    s[i] = i == 0 ? bc0(so) : i == 1 ? bc1(so) : bc2(so);
    c[i] = i == 0 ? bc0(co) : i == 1 ? bc1(co) : bc2(co);
    qd[i] = role == 0 ? x[NJ + i] : V(0);
    qdd[i] = V(role == i + 1 ? 1 : 0);
  }
  rnea_cv<true, true>(P, c, s, qd, qdd, tau, V(role == 0 ? 1 : 0), cmp);
  V b[NJ], M[NJ][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    // the group is a DPP row (16 lanes): row_newbcast:n (gfx90a+) hands lane n of the
    // row to all of it on the VALU, off the LDS crossbar that ds_bpermute goes through
    b[i] = qperm<QP_ROWBC + 0>(tau[i]);
#pragma unroll
    for (int k = 0; k < NJ; ++k) M[i][k] = rowbc_role(tau[i], 1 + k);
  }
  V r[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) r[i] = (i < NU ? u[i < NU ? i : 0] : V(0)) - b[i];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const V inv = crecip(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < NJ; ++i) {
      const V lk = M[i][k] * inv;
#pragma unroll
      for (int j = k + 1; j < NJ; ++j) M[i][j] = M[i][j] - lk * M[k][j];
      r[i] = r[i] - lk * r[k];
    }
  }
  V q2[NJ];
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    V acc = r[i];
#pragma unroll
    for (int j = i + 1; j < NJ; ++j) acc = acc - M[i][j] * q2[j];
    q2[i] = acc * crecip(M[i][i]);
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    xd[i] = x[NJ + i];
    xd[NJ + i] = q2[i];
  }
}

// lane l ^ 16 of a 32-lane group (the other DPP row of the group): ds_swizzle in bit
// mode, and 0x1F, or 0, xor 0x10 — a crossbar move, no LDS memory
__device__ __forceinline__ double swap_rows(double x) {
  const u2v p = __builtin_bit_cast(u2v, x);
  const u2v q = {(unsigned)__builtin_amdgcn_ds_swizzle((int)p.x, 0x401F),
                 (unsigned)__builtin_amdgcn_ds_swizzle((int)p.y, 0x401F)};
  return __builtin_bit_cast(double, q);
}

// chain_xdot over a 32-lane group (four to seven joints: NJ + 1 passes do not fit the four
// roles of a 16-lane group, and eight joints' nine do not fit this one's eight): eight quads,
// lane 4·role + c as in rnea_cv — role 0 the bias, roles 1..NJ the columns of M, the rest
// idle passes (q̇ = q̈ = g = 0). The group is two DPP rows.
//  * sin/cos: lane n of EACH row evaluates joint min(n, NJ − 1), and row_newbcast:i hands
//    joint i's pair to the row — one polynomial pair per lane, no cross-row traffic;
//  * b and M: the rows swap their τ once (swap_rows); after it both rows hold the even
//    row's τ (roles 0..3: b and columns 0..2) and the odd row's (roles 4..NJ: columns
//    3..NJ − 1) and row_newbcast picks lane 4·(role mod 4) of either.
// Every lane then eliminates the same NJ×NJ system in the scalar pass's order.
template <int NJ, int NU>
__device__ __forceinline__ void chain_xdot_cv32(const ChainK<double, NJ>& P, const double (&x)[2 * NJ],
                                                const double (&u)[NU], double (&xd)[2 * NJ]) {
  using V = double;
  static_assert(NJ + 1 <= 8 && NJ > 3, "one role per pass in a group of 32");
  // the evaluation re-reads the chain constants from LDS: kept in registers across the
  // four RK4 stages (≈160 lane-dependent doubles) they spill
  asm volatile("" ::: "memory");
  const int l32 = threadIdx.x & 31;
  const int role = l32 >> 2, cmp = l32 & 3, n16 = l32 & 15;
  const bool odd = (l32 & 16) != 0;
  V c[NJ], s[NJ], qd[NJ], qdd[NJ], tau[NJ];
  V ang = x[0];
#pragma unroll
  for (int i = 1; i < NJ; ++i) {
    // an opaque copy: a select between two elements of x is otherwise folded into a load
    // at a selected address, and x stays an array in scratch for it
    V xi = x[i];
    asm volatile("" : "+v"(xi));
    if (n16 >= i) ang = xi;
  }
  // fast_sincos with the large-argument fallback in line: a call here (big_sincos) hands
  // its results back through scratch and the live registers around it through spills
  V so, co;
  if (__builtin_expect(fabs(ang) > 1e5, 0)) sincos(ang, &so, &co);
  else sincos_reduced(ang, so, co);
  // lane n of the row (n a constant after unrolling). The callers ask for lanes 0..NJ − 1
  // (a joint's sin/cos) and 0, 4, 8, 12 (component 0 of a role): with NJ ≤ 7 that is
  // 0..6, 8 and 12, the cases below
  auto rowlane = [](V v, int n) {
    switch (n) {
      case 0: return qperm<QP_ROWBC + 0>(v);
      case 1: return qperm<QP_ROWBC + 1>(v);
      case 2: return qperm<QP_ROWBC + 2>(v);
      case 3: return qperm<QP_ROWBC + 3>(v);
      case 4: return qperm<QP_ROWBC + 4>(v);
      case 5: return qperm<QP_ROWBC + 5>(v);
      case 6: return qperm<QP_ROWBC + 6>(v);
      case 8: return qperm<QP_ROWBC + 8>(v);
      default: return qperm<QP_ROWBC + 12>(v);
    }
  };
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    s[i] = rowlane(so, i);
    c[i] = rowlane(co, i);
    qd[i] = role == 0 ? x[NJ + i] : V(0);
    qdd[i] = V(role == i + 1 ? 1 : 0);
  }
  rnea_cv<true, true>(P, c, s, qd, qdd, tau, V(role == 0 ? 1 : 0), cmp);
  V b[NJ], M[NJ][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const V other = swap_rows(tau[i]);
    const V ev = odd ? other : tau[i], od = odd ? tau[i] : other;
    b[i] = rowlane(ev, 0);
#pragma unroll
    for (int k = 0; k < NJ; ++k) M[i][k] = rowlane(k + 1 < 4 ? ev : od, 4 * ((k + 1) & 3));
  }
  V r[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) r[i] = (i < NU ? u[i < NU ? i : 0] : V(0)) - b[i];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const V inv = crecip(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < NJ; ++i) {
      const V lk = M[i][k] * inv;
#pragma unroll
      for (int j = k + 1; j < NJ; ++j) M[i][j] = M[i][j] - lk * M[k][j];
      r[i] = r[i] - lk * r[k];
    }
  }
  V q2[NJ];
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    V acc = r[i];
#pragma unroll
    for (int j = i + 1; j < NJ; ++j) acc = acc - M[i][j] * q2[j];
    q2[i] = acc * crecip(M[i][i]);
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    xd[i] = x[NJ + i];
    xd[NJ + i] = q2[i];
  }
}

// RK4 (chain_rk4's arithmetic and association: x + ⅙(((k₁ + 2k₂) + 2k₃) + k₄)) on the
// 32-lane evaluation, the four stages as a loop: one evaluation is ≈1,900 instructions,
// and unrolled the step neither fits the registers (the scheduler interleaves the stages'
// DPP moves and constant reads) nor sits well in the instruction cache.
template <int NJ, int NU>
__device__ __forceinline__ void chain_rk4_cv32(const ChainK<double, NJ>& P, const double (&x)[2 * NJ],
                                               const double (&u)[NU], double (&out)[2 * NJ]) {
  constexpr int NX = 2 * NJ;
  double y[NX], acc[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) y[i] = x[i];
#pragma nounroll
  for (int st = 0; st < 4; ++st) {
    double k[NX];
    chain_xdot_cv32<NJ, NU>(P, y, u, k);
    const double wy = st == 2 ? 1.0 : 0.5;             // x + ½k₁, x + ½k₂, x + k₃
    const double wa = (st == 0 || st == 3) ? 1.0 : 2.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      k[i] = P.dt * k[i];
      acc[i] = st == 0 ? k[i] : acc[i] + wa * k[i];
      y[i] = x[i] + wy * k[i];
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) out[i] = x[i] + (1.0 / 6.0) * acc[i];
}

// ---------------------------------------------------------------------------
// Closed-form dynamics of a 2-joint fixed-base chain (round 2, the default for the
// iteration kernels of 2-joint chains). M(q) depends on q₂ only (turning the whole
// chain about joint 1's fixed axis preserves its kinetic energy) and is a trigonometric
// polynomial of degree 2 in q₂ (body 2's rotation enters its kinetic energy
// quadratically, every factor affine in cos q₂, sin q₂); the gravity torque ∂V/∂q is
// bilinear in (1, cos q₁, sin q₁) ⊗ (1, cos q₂, sin q₂) (each COM's height is). The
// coefficients are sampled from the recursive Newton-Euler above, in fp64, when the
// handle is created — M at 5 angles, g on a 3×3 grid: the discrete Fourier transform is
// exact for these degrees — and the result is checked against the recursion at random
// states before it is used (chain_trig_check_kernel). The velocity term is the
// Christoffel form of M′ = dM/dq₂: c = q̇₂·M′q̇ − ½ e₂ q̇ᵀM′q̇. The same f(x, u) as the
// recursion (RBD_helper_functions.jl:61-66), ≈60 operations and two sin/cos instead
// of the three Newton-Euler passes; the rounding differs.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// cost_functions.jl's task-space final cost (src/cost_functions.jl:5-27, the device side
// of ilqr_chain_set_simple_costs): ℓ_f(x) = w Σ_k (p_k(q) − t_k)² where p is the root-
// frame position of a point fixed on one body. Through two revolute joints each
// coordinate is bilinear in (1, cos q₁, sin q₁) ⊗ (1, cos q₂, sin q₂) (Rodrigues is
// affine in cos, sin of each angle), so the handle stores the coefficients, sampled from
// the kinematics on the 3×3 grid like g's. The reference's reading takes the point's z
// for every k (work_space_traj[end] .- transpose(final_target), :21): the handle then
// stores z's coefficients in all three rows. Lives in device memory (one pointer in the
// kernel arguments; read only when the cost mode is set).
// ---------------------------------------------------------------------------
struct ChainTask {
  double Pc[3][3][3];  // p_k = Σ_ab Pc[k][a][b] φ_a(q₁) φ_b(q₂), φ = (1, cos, sin)
  double t[3];         // final_target
  double w;            // weight
};

// ℓ_f(q) in V (the forward's final cost, forward_pass.jl:192); the sum runs in the
// reference's order: weight · ((e₁² + e₂²) + e₃²) (cost_functions.jl:21-23)
template <class V>
__device__ __forceinline__ V chain_task_cost(const ChainTask* __restrict__ C, V q0, V q1) {
  V s0, c0, s1, c1;
  vsincos(q0, s0, c0);
  vsincos(q1, s1, c1);
  V acc = V(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    V h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      h[a] = (V)C->Pc[k][a][0] + ((V)C->Pc[k][a][1] * c1 + (V)C->Pc[k][a][2] * s1);
    const V e = (h[0] + (h[1] * c0 + h[2] * s0)) - (V)C->t[k];
    acc = acc + e * e;
  }
  return (V)C->w * acc;
}

// ∇ℓ_f and ∇²ℓ_f on (q₁, q₂) in f64 (final_cost_quadratization, backward_pass.jl:134-153):
// 2w Σ_k e_k ∇p_k and 2w Σ_k (∇p_k ∇p_kᵀ + e_k ∇²p_k), e_k = p_k − t_k. H = (H₁₁, H₁₂, H₂₂).
__device__ __forceinline__ void chain_task_quad(const ChainTask* __restrict__ C, double q0, double q1,
                                                double (&g)[2], double (&H)[3]) {
  double s0, c0, s1, c1;
  vsincos(q0, s0, c0);
  vsincos(q1, s1, c1);
  g[0] = g[1] = H[0] = H[1] = H[2] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double h[3], hd[3], hdd[3];  // φ(q₂), φ′(q₂), φ″(q₂) contracted with the q₂ index
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double* r = C->Pc[k][a];
      h[a] = r[0] + (r[1] * c1 + r[2] * s1);
      hd[a] = r[2] * c1 - r[1] * s1;
      hdd[a] = -(r[1] * c1 + r[2] * s1);
    }
    const double p = h[0] + (h[1] * c0 + h[2] * s0);
    const double p0 = h[2] * c0 - h[1] * s0, p1 = hd[0] + (hd[1] * c0 + hd[2] * s0);
    const double p00 = -(h[1] * c0 + h[2] * s0), p01 = hd[2] * c0 - hd[1] * s0;
    const double p11 = hdd[0] + (hdd[1] * c0 + hdd[2] * s0);
    const double e = p - C->t[k];
    g[0] += e * p0;
    g[1] += e * p1;
    H[0] += p0 * p0 + e * p00;
    H[1] += p0 * p1 + e * p01;
    H[2] += p1 * p1 + e * p11;
  }
  const double w2 = 2.0 * C->w;
  g[0] *= w2;
  g[1] *= w2;
  H[0] *= w2;
  H[1] *= w2;
  H[2] *= w2;
}

template <class V>
struct ChainTrig {
  V Mc[3][5];     // M₀₀, M₀₁, M₁₁: a₀ + a₁ cos q₂ + b₁ sin q₂ + a₂ cos 2q₂ + b₂ sin 2q₂
  V Gc[2][3][3];  // g_i = Σ_ab Gc[i][a][b] φ_a(q₁) φ_b(q₂), φ = (1, cos, sin)
  V dt;
  V tgt[2], qw[2], rw[2], qfw[2];  // joint-space cost (as ChainK)
  const ChainTask* task;           // the task-space final cost in place of qfw's, or null
};

// q̈ from sin/cos of both joint angles, q̇ = (w0, w1) and u
template <int NU, class S, class V>
__device__ __forceinline__ void chain_qdd_trig(const ChainTrig<V>& P, const S& s1, const S& c1, const S& s2,
                                               const S& c2, const S& w0, const S& w1, const S (&u)[NU],
                                               S& a0, S& a1) {
  S m[3], dm[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    // M_e = a₀ + a₁ cos + b₁ sin + a₂ cos 2q + b₂ sin 2q and dM_e/dq₂ = b₁ cos − a₁ sin +
    // 2(b₂ cos 2q − a₂ sin 2q) in Horner form in (cos q₂, sin q₂), as chain_qdd_trig2 (the
    // kernel argument holds M's coefficients only: fewer scalar registers than a second table)
    const V a0 = P.Mc[e][0], a1 = P.Mc[e][1], b1 = P.Mc[e][2], a2 = P.Mc[e][3], b2 = P.Mc[e][4];
    m[e] = (a0 - a2) + c2 * ((a1 + (V(2) * a2) * c2) + (V(2) * b2) * s2) + b1 * s2;
    dm[e] = V(-2) * b2 + c2 * ((b1 + (V(4) * b2) * c2) - (V(4) * a2) * s2) - a1 * s2;
  }
  S g[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    S h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) h[a] = P.Gc[i][a][0] + (P.Gc[i][a][1] * c2 + P.Gc[i][a][2] * s2);
    g[i] = h[0] + (h[1] * c1 + h[2] * s1);
  }
  const S p0 = dm[0] * w0 + dm[1] * w1, p1 = dm[1] * w0 + dm[2] * w1;  // M′q̇
  const S qq = w0 * p0 + w1 * p1;                                      // q̇ᵀM′q̇
  S r0 = u[0] - (w1 * p0 + g[0]);
  S r1 = (w1 * p1 - V(0.5) * qq) + g[1];
  if constexpr (NU > 1) r1 = u[NU - 1] - r1;
  else r1 = -r1;
  const S det = m[0] * m[2] - m[1] * m[1];
  const S id = crecip(det);
  a0 = (m[2] * r0 - m[1] * r1) * id;
  a1 = (m[0] * r1 - m[1] * r0) * id;
}

template <int NU, class S, class V>
__device__ __forceinline__ void chain_xdot_trig(const ChainTrig<V>& P, const S (&x)[4], const S (&u)[NU],
                                                S (&xd)[4]) {
  S s1, c1, s2, c2;
  scs(x[0], s1, c1);
  scs(x[1], s2, c2);
  xd[0] = x[2];
  xd[1] = x[3];
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, x[2], x[3], u, xd[2], xd[3]);
}

// One RK4 step of the closed form without a branch (the forward's fast path, as the
// 2-link's rk4_roll): stage 1 reduces both angles, stages 2-4 shift their sin/cos by
// h = ½k₁, ½k₂, k₃ (|h| ≤ 1/8); `bad` flags |h| > 1/8 or an angle past the reduction's
// range, and the caller redoes the rollout on chain_rk4 (NaN: not flagged, NaN either way)
// sin/cos of both joint angles carried from step to step (the forward group's carry): the
// step's stage 1 reads them and leaves those of the new state by the stages' angle shift
template <class V>
struct ChainCarry {
  V s[2], c[2];
};

template <int NU, class V>
__device__ __forceinline__ void chain_trig_rk4_fast(const ChainTrig<V>& P, const V (&x)[4], const V (&u)[NU],
                                                    V (&out)[4], bool& bad, ChainCarry<V>& cy) {
  const V h = V(0.5);
  V s1, c1, s2, c2, a0, a1;
  const V s10 = cy.s[0], c10 = cy.c[0], s20 = cy.s[1], c20 = cy.c[1];
  chain_qdd_trig<NU>(P, s10, c10, s20, c20, x[2], x[3], u, a0, a1);
  const V k10 = P.dt * x[2], k11 = P.dt * x[3], k12 = P.dt * a0, k13 = P.dt * a1;
  V y2 = x[2] + h * k12, y3 = x[3] + h * k13;
  sincos_shift_t(s10, c10, h * k10, s1, c1);
  sincos_shift_t(s20, c20, h * k11, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const V k20 = P.dt * y2, k21 = P.dt * y3, k22 = P.dt * a0, k23 = P.dt * a1;
  y2 = x[2] + h * k22;
  y3 = x[3] + h * k23;
  sincos_shift_t(s10, c10, h * k20, s1, c1);
  sincos_shift_t(s20, c20, h * k21, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const V k30 = P.dt * y2, k31 = P.dt * y3, k32 = P.dt * a0, k33 = P.dt * a1;
  y2 = x[2] + k32;
  y3 = x[3] + k33;
  sincos_shift_t(s10, c10, k30, s1, c1);
  sincos_shift_t(s20, c20, k31, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const V k40 = P.dt * y2, k41 = P.dt * y3, k42 = P.dt * a0, k43 = P.dt * a1;
  const V sixth = V(1) / V(6);
  out[0] = x[0] + sixth * (((k10 + V(2) * k20) + V(2) * k30) + k40);
  out[1] = x[1] + sixth * (((k11 + V(2) * k21) + V(2) * k31) + k41);
  out[2] = x[2] + sixth * (((k12 + V(2) * k22) + V(2) * k32) + k42);
  out[3] = x[3] + sixth * (((k13 + V(2) * k23) + V(2) * k33) + k43);
  const V h0 = out[0] - x[0], h1 = out[1] - x[1];
  sincos_shift_t(s10, c10, h0, cy.s[0], cy.c[0]);
  sincos_shift_t(s20, c20, h1, cy.s[1], cy.c[1]);
  const V hm = fmax(fmax(fmax(fabs(k10), fabs(k11)), fmax(fabs(k20), fabs(k21))),
                    V(2) * fmax(fmax(fabs(k30), fabs(k31)), fmax(fabs(h0), fabs(h1))));
  bad |= ((int)(hm > V(0.25)) | (int)(fabs(x[0]) > ReducedRange<V>::v) | (int)(fabs(x[1]) > ReducedRange<V>::v)) != 0;
}

// ---------------------------------------------------------------------------
// The fp32 fast step with the two joints packed (v_pk_* arithmetic on (joint 1,
// joint 2) pairs: the angle reductions and shifts, M's diagonal, g, M′q̇, the solve and
// the RK4 glue), the configuration BASELINE config 5 runs. The formulas of
// chain_trig_rk4_fast per component (FMA contraction may place roundings differently).
// ---------------------------------------------------------------------------
__device__ __forceinline__ F2 f2fma(F2 a, F2 b, F2 c) { return __builtin_elementwise_fma(a, b, c); }

// sincos_shift_t (fp32) on both components
__device__ __forceinline__ void sincos2_shift(F2 s0, F2 c0, F2 h, F2& s, F2& c) {
  const F2 z = h * h;
  const F2 sh = f2fma(h * z, f2fma(z, F2(1.0f / 120.0f), F2(-1.0f / 6.0f)), h);
  const F2 ch = f2fma(z, f2fma(z, F2(1.0f / 24.0f), F2(-0.5f)), F2(1.0f));
  s = f2fma(s0, ch, c0 * sh);
  c = f2fma(c0, ch, -(s0 * sh));
}

// q̈ (both joints) from packed sin/cos (joint 1, joint 2), q̇ and u
template <int NU>
__device__ __forceinline__ F2 chain_qdd_trig2(const ChainTrig<float>& P, F2 sn, F2 cs, F2 w, const float (&u)[NU]) {
  const float s2 = sn.y, c2 = cs.y;
  // M's entries a₀ + a₁ cos q₂ + b₁ sin q₂ + a₂ cos 2q₂ + b₂ sin 2q₂ and their derivatives
  // b₁ cos − a₁ sin + 2(b₂ cos 2q − a₂ sin 2q), in Horner form in (cos q₂, sin q₂):
  // k₀ + c·(k₁ + k₂ c + k₃ s) + k₄ s, with M: (a₀ − a₂, a₁, 2a₂, 2b₂, b₁) and
  // dM: (−2b₂, b₁, 4b₂, −4a₂, −a₁) (loop-invariant coefficient pairs)
  auto horner = [&](F2 k0, F2 k1, F2 k2, F2 k3, F2 k4) {
    const F2 in = f2fma(k3, F2(s2), f2fma(k2, F2(c2), k1));
    return f2fma(k4, F2(s2), f2fma(in, F2(c2), k0));
  };
  auto a0 = [&](int e) { return P.Mc[e][0]; };
  auto a1 = [&](int e) { return P.Mc[e][1]; };
  auto b1 = [&](int e) { return P.Mc[e][2]; };
  auto a2 = [&](int e) { return P.Mc[e][3]; };
  auto b2 = [&](int e) { return P.Mc[e][4]; };
  // (M₀₀, M₁₁), (M₀₁, dM₀₁/dq₂), (dM₀₀, dM₁₁) as pairs
  const F2 md = horner(F2{a0(0) - a2(0), a0(2) - a2(2)}, F2{a1(0), a1(2)}, F2{2.0f * a2(0), 2.0f * a2(2)},
                       F2{2.0f * b2(0), 2.0f * b2(2)}, F2{b1(0), b1(2)});
  const F2 mo = horner(F2{a0(1) - a2(1), -2.0f * b2(1)}, F2{a1(1), b1(1)}, F2{2.0f * a2(1), 4.0f * b2(1)},
                       F2{2.0f * b2(1), -4.0f * a2(1)}, F2{b1(1), -a1(1)});
  const F2 dmd = horner(F2{-2.0f * b2(0), -2.0f * b2(2)}, F2{b1(0), b1(2)}, F2{4.0f * b2(0), 4.0f * b2(2)},
                        F2{-4.0f * a2(0), -4.0f * a2(2)}, F2{-a1(0), -a1(2)});
  // g (both components): h_a = G[·][a][0] + G[·][a][1] cos q₂ + G[·][a][2] sin q₂
  F2 h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    h[a] = F2{P.Gc[0][a][0], P.Gc[1][a][0]} +
           (F2{P.Gc[0][a][1], P.Gc[1][a][1]} * c2 + F2{P.Gc[0][a][2], P.Gc[1][a][2]} * s2);
  const F2 g = h[0] + (h[1] * cs.x + h[2] * sn.x);
  // M′q̇ = (dM₀₀ w₀ + dM₀₁ w₁, dM₀₁ w₀ + dM₁₁ w₁), packed
  const F2 p = f2fma(F2{mo.y, mo.y}, w.yx, dmd * w);
  const float qq = w.x * p.x + w.y * p.y;
  const F2 t = f2fma(F2{w.y, w.y}, p, g);  // (w₁p₀ + g₀, w₁p₁ + g₁)
  const float r0 = u[0] - t.x;
  float r1 = t.y - 0.5f * qq;
  if constexpr (NU > 1) r1 = u[NU - 1] - r1;
  else r1 = -r1;
  const float det = md.x * md.y - mo.x * mo.x;
  const float id = crecip(det);
  // M⁻¹r = (M₁₁ r₀ − M₀₁ r₁, M₀₀ r₁ − M₀₁ r₀) / det, packed
  const F2 r{r0, r1};
  return (md.yx * r - F2{mo.x, mo.x} * r.yx) * id;
}

template <int NU>
__device__ __forceinline__ void chain_trig_rk4_fast2(const ChainTrig<float>& P, const float (&x)[4],
                                                     const float (&u)[NU], float (&out)[4], bool& bad,
                                                     ChainCarry<float>& cy) {
  const F2 q{x[0], x[1]}, w{x[2], x[3]};
  const float dt = P.dt;
  const F2 s0{cy.s[0], cy.s[1]}, c0{cy.c[0], cy.c[1]};
  F2 sn, cs;
  F2 a = chain_qdd_trig2<NU>(P, s0, c0, w, u);
  const F2 k1p = dt * w, k1v = dt * a;
  F2 y = w + 0.5f * k1v;
  sincos2_shift(s0, c0, 0.5f * k1p, sn, cs);
  a = chain_qdd_trig2<NU>(P, sn, cs, y, u);
  const F2 k2p = dt * y, k2v = dt * a;
  y = w + 0.5f * k2v;
  sincos2_shift(s0, c0, 0.5f * k2p, sn, cs);
  a = chain_qdd_trig2<NU>(P, sn, cs, y, u);
  const F2 k3p = dt * y, k3v = dt * a;
  y = w + k3v;
  sincos2_shift(s0, c0, k3p, sn, cs);
  a = chain_qdd_trig2<NU>(P, sn, cs, y, u);
  const F2 k4p = dt * y, k4v = dt * a;
  const float sixth = 1.0f / 6.0f;
  const F2 op = q + sixth * (((k1p + 2.0f * k2p) + 2.0f * k3p) + k4p);
  const F2 ov = w + sixth * (((k1v + 2.0f * k2v) + 2.0f * k3v) + k4v);
  out[0] = op.x; out[1] = op.y; out[2] = ov.x; out[3] = ov.y;
  const F2 hq = op - q;  // the carry: sin/cos of the new angles
  F2 sq, cq;
  sincos2_shift(s0, c0, hq, sq, cq);
  cy.s[0] = sq.x; cy.s[1] = sq.y; cy.c[0] = cq.x; cy.c[1] = cq.y;
  const F2 m1 = __builtin_elementwise_max(__builtin_elementwise_abs(k1p), __builtin_elementwise_abs(k2p));
  const F2 m2 = __builtin_elementwise_max(__builtin_elementwise_max(m1, 2.0f * __builtin_elementwise_abs(k3p)),
                                          2.0f * __builtin_elementwise_abs(hq));
  const float hm = fmaxf(m2.x, m2.y);
  bad |= ((int)(hm > 0.25f) | (int)(fabsf(x[0]) > 8192.0f) | (int)(fabsf(x[1]) > 8192.0f)) != 0;
}

// the chain's closed form as a model of the shared forward group (ilqr_fwd_group.h)
template <class V_, int NU_>
struct ChainTrigModel {
  using V = V_;
  static constexpr int NU = NU_;
  static constexpr bool HAS_FAST = true;
  static constexpr bool HAS_CARRY = true;
  using Carry = ChainCarry<V>;
  ChainTrig<V> P;
  __device__ __forceinline__ Carry carry_init(const V (&x)[4]) const {
    Carry k;
    sincos_red_t(x[0], k.s[0], k.c[0]);
    sincos_red_t(x[1], k.s[1], k.c[1]);
    return k;
  }
  __device__ __forceinline__ void rk4_fast(const V (&x)[4], const V (&u)[NU], V (&o)[4], bool& bad,
                                           Carry& k) const {
    // fp32: the joints packed (v_pk_* pairs)
    if constexpr (std::is_same_v<V, float>) chain_trig_rk4_fast2<NU>(P, x, u, o, bad, k);
    else chain_trig_rk4_fast<NU>(P, x, u, o, bad, k);
  }
  __device__ __forceinline__ void rk4_robust(const V (&x)[4], const V (&u)[NU], V (&o)[4]) const;
  // ℓ(x̄ₖ − x_trajₖ, ūₖ) on the joints (forward_pass.jl:187-190; RBD_helper_functions.jl:85-99)
  __device__ __forceinline__ V stage_cost(const V (&xb)[4], const V (&xt)[4], V xtw, const V (&ub)[NU]) const {
    V lk = V(0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const V e = P.tgt[i] - fma(-xtw, xt[i], xb[i]);
      lk = fma(P.qw[i] * e, e, lk);
    }
#pragma unroll
    for (int a = 0; a < NU; ++a) lk = fma(P.rw[a] * ub[a], ub[a], lk);
    return lk;
  }
  // final_cost(x̄_N) on the raw state (:192; RBD_helper_functions.jl:105-116)
  __device__ __forceinline__ V final_cost(const V (&xb)[4]) const {
    if (P.task) return chain_task_cost<V>(P.task, xb[0], xb[1]);  // cost_functions.jl:16-24
    V lf = V(0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const V e = P.tgt[i] - xb[i];
      lf = fma(P.qfw[i] * e, e, lf);
    }
    return lf;
  }
};

// RK4 (RBD_helper_functions.jl:70-78) on either parameter set: ChainK (the recursion;
// SPLIT = the 16-lane component-parallel form) or ChainTrig (closed form, 2 joints)
template <int NJ, int NU, bool SPLIT = false, class S, class PK>
__device__ __forceinline__ void chain_rk4(const PK& P, const S (&x)[2 * NJ],
                                          const S (&u)[NU], S (&out)[2 * NJ]) {
  constexpr int NX = 2 * NJ;
  using V = decltype(P.dt);
  auto xdot = [](const PK& Pc, const S (&xx)[2 * NJ], const S (&uu)[NU], S (&o)[2 * NJ]) {
    if constexpr (std::is_same_v<PK, ChainTrig<V>>)
      chain_xdot_trig<NU>(Pc, xx, uu, o);
    else if constexpr (SPLIT)
      chain_xdot_cv<NJ, NU>(Pc, xx, uu, o);
    else
      chain_xdot<NJ, NU>(Pc, xx, uu, o);
  };
  S k1[NX], k2[NX], k3[NX], k4[NX], y[NX];
  const V h = V(0.5);
  xdot(P, x, u, k1);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    k1[i] = P.dt * k1[i];
    y[i] = x[i] + h * k1[i];
  }
  xdot(P, y, u, k2);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    k2[i] = P.dt * k2[i];
    y[i] = x[i] + h * k2[i];
  }
  xdot(P, y, u, k3);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    k3[i] = P.dt * k3[i];
    y[i] = x[i] + k3[i];
  }
  xdot(P, y, u, k4);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    k4[i] = P.dt * k4[i];
    out[i] = x[i] + (V(1) / V(6)) * (((k1[i] + V(2) * k2[i]) + V(2) * k3[i]) + k4[i]);
  }
}

template <class V_, int NU_>
__device__ __forceinline__ void ChainTrigModel<V_, NU_>::rk4_robust(const V (&x)[4], const V (&u)[NU],
                                                                   V (&o)[4]) const {
  chain_rk4<2, NU>(P, x, u, o);
}

// ---------------------------------------------------------------------------
// f(x, u) for n points (a rollout primitive and the dynamics parity test)
// ---------------------------------------------------------------------------
template <class V, int NJ, int NU, class PK = ChainK<V, NJ>>
__global__ __launch_bounds__(256) void chain_dynamics_kernel(PK P, int n,
                                                             const V* __restrict__ x,
                                                             const V* __restrict__ u,
                                                             V* __restrict__ xo) {
  constexpr int NX = 2 * NJ;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  V xs[NX], us[NU], o[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) xs[k] = x[(size_t)i * NX + k];
#pragma unroll
  for (int k = 0; k < NU; ++k) us[k] = u[(size_t)i * NU + k];
  chain_rk4<NJ, NU>(P, xs, us, o);
#pragma unroll
  for (int k = 0; k < NX; ++k) xo[(size_t)i * NX + k] = o[k];
}

// The central-difference pair f(z + h e_k), f(z − h e_k) of the fp32 closed form in one
// packed RK4 (F2 = (+, −)): stage 1 takes both angles' sin/cos in full, stages 2-4 shift
// them by ½k₁, ½k₂, k₃ (sincos2_shift, |h| ≤ 1/8) instead of reducing the stage's angle
// again. `bad` flags a larger shift; the caller then evaluates the pair on chain_rk4.
template <int NU>
__device__ __forceinline__ void chain_trig_rk4_pm(const ChainTrig<float>& P, const F2 (&x)[4], const F2 (&u)[NU],
                                                  F2 (&out)[4], bool& bad) {
  const float dt = P.dt;
  F2 s10, c10, s20, c20, s1, c1, s2, c2, a0, a1;
  scs(x[0], s10, c10);
  scs(x[1], s20, c20);
  chain_qdd_trig<NU>(P, s10, c10, s20, c20, x[2], x[3], u, a0, a1);
  const F2 k10 = dt * x[2], k11 = dt * x[3], k12 = dt * a0, k13 = dt * a1;
  F2 y2 = x[2] + 0.5f * k12, y3 = x[3] + 0.5f * k13;
  sincos2_shift(s10, c10, 0.5f * k10, s1, c1);
  sincos2_shift(s20, c20, 0.5f * k11, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const F2 k20 = dt * y2, k21 = dt * y3, k22 = dt * a0, k23 = dt * a1;
  y2 = x[2] + 0.5f * k22;
  y3 = x[3] + 0.5f * k23;
  sincos2_shift(s10, c10, 0.5f * k20, s1, c1);
  sincos2_shift(s20, c20, 0.5f * k21, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const F2 k30 = dt * y2, k31 = dt * y3, k32 = dt * a0, k33 = dt * a1;
  y2 = x[2] + k32;
  y3 = x[3] + k33;
  sincos2_shift(s10, c10, k30, s1, c1);
  sincos2_shift(s20, c20, k31, s2, c2);
  chain_qdd_trig<NU>(P, s1, c1, s2, c2, y2, y3, u, a0, a1);
  const F2 k40 = dt * y2, k41 = dt * y3, k42 = dt * a0, k43 = dt * a1;
  const float sixth = 1.0f / 6.0f;
  out[0] = x[0] + sixth * (((k10 + 2.0f * k20) + 2.0f * k30) + k40);
  out[1] = x[1] + sixth * (((k11 + 2.0f * k21) + 2.0f * k31) + k41);
  out[2] = x[2] + sixth * (((k12 + 2.0f * k22) + 2.0f * k32) + k42);
  out[3] = x[3] + sixth * (((k13 + 2.0f * k23) + 2.0f * k33) + k43);
  const F2 m1 = __builtin_elementwise_max(
      __builtin_elementwise_max(__builtin_elementwise_abs(k10), __builtin_elementwise_abs(k11)),
      __builtin_elementwise_max(__builtin_elementwise_abs(k20), __builtin_elementwise_abs(k21)));
  const F2 m2 = __builtin_elementwise_max(
      m1, 2.0f * __builtin_elementwise_max(__builtin_elementwise_abs(k30), __builtin_elementwise_abs(k31)));
  bad |= fmaxf(m2.x, m2.y) > 0.25f;
}

// ---------------------------------------------------------------------------
// Linearisation record per (b, t): [A | B] (NX × (NX+NU), row-major), x_t, u_t
// ---------------------------------------------------------------------------
template <int NJ, int NU>
struct Rec {
  static constexpr int NX = 2 * NJ;
  static constexpr int NJAC = NX * (NX + NU);
  static constexpr int N = NJAC + NX + NU;
};

// One lane per (b, t, direction k): lane g = (b·T + t)·ND + k, so a record's ND
// columns come from ND adjacent lanes and a block writes a contiguous run of records.
// (v7 ran one lane per (b, t) over all ND directions: 3,200 waves at B=2048, T=100 on a
// 3-wave/SIMD occupancy — a second, nearly empty round on 32 CUs.)
// occupancy asked of the linearisation: central differences, the ±h pair packed
// (one packed evaluation), at 3 waves/SIMD (168 VGPRs; config 5 2,208 it/s against 2,175
// at 2 waves, 1,962 at 4 where it spills, and 2,163 unpacked at 4 waves); the dual
// kernel at 2 (256 VGPRs, ~150 spilled, still faster than 1 wave with 300 registers:
// config 5 dual 1,710 → 1,908 it/s)
constexpr int CHAIN_FD_WAVES = 3, CHAIN_DUAL_WAVES = 2;
template <class V, int NJ, int NU, int LIN, class PK = ChainK<V, NJ>>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LIN == ILQR_LINEARIZE_CENTRAL_FD ? CHAIN_FD_WAVES : CHAIN_DUAL_WAVES))) void chain_linearize_kernel(PK P, int B, int T,
                                                              const V* __restrict__ x,
                                                              const V* __restrict__ u,
                                                              const int32_t* __restrict__ status,
                                                              V* __restrict__ J) {
  constexpr int NX = 2 * NJ, ND = NX + NU, NR = Rec<NJ, NU>::N;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * T * ND) return;
  const int bt = (int)(g / ND);
  const int kd = (int)(g - (size_t)bt * ND);
  const int b = bt / T, t = bt - b * T;
  if (status && status[b] != ILQR_TRAJ_OK) return;
  const V* xb = x + ((size_t)b * (T + 1) + t) * NX;
  const V* ub = u + ((size_t)b * T + t) * NU;
  V* Jt = J + ((size_t)b * T + t) * NR;
  V z[ND];
#pragma unroll
  for (int k = 0; k < NX; ++k) z[k] = xb[k];
#pragma unroll
  for (int k = 0; k < NU; ++k) z[NX + k] = ub[k];
  if constexpr (LIN == ILQR_LINEARIZE_DUAL) {
    // the reference's two ForwardDiff.jacobian calls, one direction per lane (this
    // lane's column k of [A | B]; a pass carrying all ND directions would spill:
    // ≈4.6 KB of scratch per lane)
    constexpr int DC = 1;
    using D = DualT<DC, V>;
    {
      const int k0 = kd;
      D xs[NX], us[NU], o[NX];
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        D v(z[k]);
#pragma unroll
        for (int c = 0; c < DC; ++c) v.d[c] = (k == k0 + c) ? V(1) : V(0);
        if (k < NX) xs[k] = v; else us[k - NX] = v;
      }
      chain_rk4<NJ, NU>(P, xs, us, o);
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int c = 0; c < DC; ++c)
          if (k0 + c < ND) Jt[i * ND + k0 + c] = o[i].d[c];
    }
  } else {
    // central differences, step h = ε^(1/3)·max(1, |z_k|), divided by the step actually taken
    const V cbe = sizeof(V) == 4 ? V(4.921566e-3) : V(6.0554544523933395e-6);
    {
      const int k = kd;
      V zk = z[0];
#pragma unroll
      for (int j = 1; j < ND; ++j)
        if (j == k) zk = z[j];
      const V h = cbe * fmax(V(1), fabs(zk));
      V xp[NX], up[NU], xm[NX], um[NU], fp[NX], fm[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) xp[j] = xm[j] = z[j];
#pragma unroll
      for (int j = 0; j < NU; ++j) up[j] = um[j] = z[NX + j];
      V zp = zk + h, zm = zk - h;
#pragma unroll
      for (int j = 0; j < NX; ++j)
        if (j == k) { xp[j] = zp; xm[j] = zm; }
#pragma unroll
      for (int j = 0; j < NU; ++j)
        if (NX + j == k) { up[j] = zp; um[j] = zm; }
      if constexpr (sizeof(V) == 4) {
        // f(z + h e_k) and f(z − h e_k) run the same instruction stream: one packed
        // evaluation (v_pk_* on the pair)
        F2 x2[NX], u2[NU], f2[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) x2[j] = F2{(float)xp[j], (float)xm[j]};
#pragma unroll
        for (int j = 0; j < NU; ++j) u2[j] = F2{(float)up[j], (float)um[j]};
        if constexpr (std::is_same_v<PK, ChainTrig<float>>) {
          bool bad = false;
          chain_trig_rk4_pm<NU>(P, x2, u2, f2, bad);
          if (bad) chain_rk4<NJ, NU>(P, x2, u2, f2);
        } else {
          chain_rk4<NJ, NU>(P, x2, u2, f2);
        }
#pragma unroll
        for (int j = 0; j < NX; ++j) { fp[j] = f2[j].x; fm[j] = f2[j].y; }
      } else {
        chain_rk4<NJ, NU>(P, xp, up, fp);
        chain_rk4<NJ, NU>(P, xm, um, fm);
      }
      const V inv = V(1) / (zp - zm);
#pragma unroll
      for (int i = 0; i < NX; ++i) Jt[i * ND + k] = (fp[i] - fm[i]) * inv;
    }
  }
  V zd = z[0];
#pragma unroll
  for (int j = 1; j < ND; ++j)
    if (j == kd) zd = z[j];
  Jt[Rec<NJ, NU>::NJAC + kd] = zd;
}

// record → separate A (B,T,NX,NX), B (B,T,NX,NU) tiles (ilqr_chain_linearize)
template <class V, int NJ, int NU>
__global__ __launch_bounds__(256) void chain_unpack_kernel(int B, int T, const V* __restrict__ J,
                                                           V* __restrict__ A, V* __restrict__ Bm) {
  constexpr int NX = 2 * NJ, ND = NX + NU, NR = Rec<NJ, NU>::N;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * T) return;
  const V* Jt = J + i * NR;
#pragma unroll
  for (int r = 0; r < NX; ++r) {
#pragma unroll
    for (int k = 0; k < NX; ++k) A[i * NX * NX + r * NX + k] = Jt[r * ND + k];
#pragma unroll
    for (int k = 0; k < NU; ++k) Bm[i * NX * NU + r * NU + k] = Jt[r * ND + NX + k];
  }
}

// ---------------------------------------------------------------------------
// Forward rollout + line search (src/forward_pass.jl:55-93), one lane per trajectory
// ---------------------------------------------------------------------------
template <class V>
struct ChainFwdOut {
  V cost;
  int trials;
  int accepted;
};

template <class V, int NJ, int NU, bool SPLIT = false, class PK = ChainK<V, NJ>>
__device__ ChainFwdOut<V> chain_forward_lane(const PK& P, int b, int T,
                                             const V* __restrict__ x, const V* __restrict__ u,
                                             const V* __restrict__ xtraj, const V* __restrict__ dg,
                                             const V* __restrict__ Kg, V prev_cost,
                                             V* __restrict__ xnew, V* __restrict__ unew, V* du2_out,
                                             const LSParams& ls) {
  constexpr int NX = 2 * NJ;
  const bool writer = !SPLIT || (threadIdx.x & 15) == 0;  // SPLIT: one lane of the group stores
  const V* xb0 = x + (size_t)b * (T + 1) * NX;
  const V* ub0 = u + (size_t)b * T * NU;
  const V* xt0 = (xtraj ? xtraj : x) + (size_t)b * (T + 1) * NX;
  const V xtw = xtraj ? V(1) : V(0);  // x_traj = NULL means zeros (forward_pass.jl:151)
  const V* d0 = dg + (size_t)b * T * NU;
  const V* K0 = Kg + (size_t)b * T * NU * NX;
  V* xo = xnew + (size_t)b * (T + 1) * NX;
  V* uo = unew + (size_t)b * T * NU;

  V alpha = V(ls.alpha0);
  ChainFwdOut<V> out{V(0), 0, 0};
  V du2 = V(0);
  for (int trial = 1; trial <= ls.max_trials; ++trial) {
    V xb[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xb[i] = xb0[i];  // x̄₁ = x₁ (:65)
    V cost = V(0);
    du2 = V(0);
    // step t's inputs (x_t, x_traj_t, K_t, u_t, δu_t) are loaded during step t − 1: a
    // step is a few µs of dependent dynamics, so the loads land off the critical path
    struct In { V xk[NX], xtk[NJ], K[NU * NX], u[NU], d[NU]; };
    auto load = [&](int t, In& in) {
#pragma unroll
      for (int i = 0; i < NX; ++i) in.xk[i] = xb0[(size_t)t * NX + i];
#pragma unroll
      for (int i = 0; i < NJ; ++i) in.xtk[i] = xt0[(size_t)t * NX + i];
#pragma unroll
      for (int k = 0; k < NU * NX; ++k) in.K[k] = K0[(size_t)t * NU * NX + k];
#pragma unroll
      for (int a = 0; a < NU; ++a) {
        in.u[a] = ub0[(size_t)t * NU + a];
        in.d[a] = d0[(size_t)t * NU + a];
      }
    };
    In cur;
    load(0, cur);
    for (int t = 0; t < T; ++t) {
      In nxt;
      load(t + 1 < T ? t + 1 : t, nxt);
      V dx[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) dx[i] = xb[i] - cur.xk[i];  // δx (:72)
      V ubar[NU];
#pragma unroll
      for (int a = 0; a < NU; ++a) {  // ūₖ = uₖ + α δuₖ + Kₖ δx (:73)
        V kdx = V(0);
#pragma unroll
        for (int i = 0; i < NX; ++i) kdx = fma(cur.K[a * NX + i], dx[i], kdx);
        const V uk = cur.u[a];
        ubar[a] = fma(alpha, cur.d[a], uk) + kdx;
        const V e = ubar[a] - uk;
        du2 = fma(e, e, du2);
      }
      // ℓ(x̄ₖ − x_trajₖ, ūₖ) (:187-190; RBD_helper_functions.jl:85-99 on the joints)
      V lk = V(0);
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        const V e = P.tgt[i] - fma(-xtw, cur.xtk[i], xb[i]);
        lk = fma(P.qw[i] * e, e, lk);
      }
#pragma unroll
      for (int a = 0; a < NU; ++a) lk = fma(P.rw[a] * ubar[a], ubar[a], lk);
      cost += lk;
#pragma unroll
      for (int i = 0; i < NX; ++i)
        if (writer) xo[(size_t)t * NX + i] = xb[i];
#pragma unroll
      for (int a = 0; a < NU; ++a)
        if (writer) uo[(size_t)t * NU + a] = ubar[a];
      V xn[NX];
      chain_rk4<NJ, NU, SPLIT>(P, xb, ubar, xn);  // x̄ₖ₊₁ = f(x̄ₖ, ūₖ) (:74)
#pragma unroll
      for (int i = 0; i < NX; ++i) xb[i] = xn[i];
      cur = nxt;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if (writer) xo[(size_t)T * NX + i] = xb[i];
    // final_cost(x̄_N) on the raw state (:192; RBD_helper_functions.jl:105-116)
    V lf = V(0);
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      const V e = P.tgt[i] - xb[i];
      lf = fma(P.qfw[i] * e, e, lf);
    }
    cost += lf;
    out.trials = trial;
    out.cost = cost;
    if (prev_cost - cost > V(0)) {  // (:77-80); NaN compares false → keep searching
      out.accepted = 1;
      break;
    }
    alpha *= V(ls.shrink);  // (:82)
  }
  if (du2_out) *du2_out = du2;
  return out;
}

template <class V>
struct ChainIter {
  const V* x;
  const V* u;
  const V* xtraj;
  V* xnew;
  V* unew;
  V* K;
  V* d;
  const V* prev_cost;
  V* new_cost;
  V* du2;
  int32_t* trials;
  int32_t* status;
  int32_t* res_parity;
  int32_t* iters;
  int parity;
  int iter;
};

// ---------------------------------------------------------------------------
// Riccati recursion of the 2-joint chain (nx = 4, nu ≤ 2) on the 4-block f64 MFMA,
// four trajectories per wave: the 2-link family's tl_backward4_wave (ilqr_twolink.hip,
// DESIGN.md §4) with the chain's weighted joint-space cost (RBD_helper_functions.jl:
// 85-116: lxx = diag(2qw, 0), luu = diag(2rw), lx = −2qw(θ* − θ), lu = 2rw·u, final
// diag(2qfw, 0) and −2qfw(θ* − θ_N)). The recursion runs in f64 whatever V is (the
// fp32 family's records and gains are converted at the load/store): one rounding of
// the gains to fp32 instead of fp32 arithmetic throughout.
template <class V>
__device__ __forceinline__ double ch_ld(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  if constexpr (sizeof(V) == 4)
    return (double)__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
  else
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
template <class V>
__device__ __forceinline__ void ch_st(double v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  if constexpr (sizeof(V) == 4)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, (float)v), r, voff, soff, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), r, voff, soff, 0);
}
__device__ __forceinline__ double ch_mf(double a, double b, double c) {  // c + aᵀb
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ double ch_mfn(double a, double b, double c) {  // c − aᵀb
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 1);
}
constexpr int CH_BW4_PF = 4;  // record prefetch depth (steps)

template <class V, int NU>
__device__ unsigned chain_backward4_wave(const ChainK<V, 2>& P, int b0, int B, unsigned active, int T,
                                         const V* __restrict__ x, const V* __restrict__ J,
                                         V* __restrict__ dg, V* __restrict__ Kg, double mu,
                                         double* lds, const ChainTask* task) {
  constexpr int NJ = 2, NX = 4, ND = NX + NU, NR = Rec<NJ, NU>::N, NJAC = Rec<NJ, NU>::NJAC;
  constexpr uint32_t DEAD = 0x80000000u, W = sizeof(V);
  b0 = __builtin_amdgcn_readfirstlane(b0);
  const int l = threadIdx.x & 63;
  const int rho = l >> 4, beta = (l >> 2) & 3, kap = l & 3;
  const int b = b0 + beta;
  const bool live = b < B && ((active >> beta) & 1u);
  const int bc = b < B ? b : B - 1;
  const int nslot = B - b0 < 4 ? B - b0 : 4;
  const bool rj = rho < NJ, ru = rho < NU;
  const int jr = rj ? rho : 0;
  const double tg = (double)P.tgt[jr], qw2 = 2.0 * (double)P.qw[jr], qfw2 = 2.0 * (double)P.qfw[jr];
  const double rw2 = ru ? 2.0 * (double)P.rw[rho < NU ? rho : 0] : 0.0;
  const double lxx = (rho == kap && rj) ? qw2 : 0.0;
  const double luu = (rho == kap && ru) ? rw2 : 0.0;
  double S = (rho == kap && rj) ? qfw2 : 0.0;
  const double xT = (double)x[((size_t)bc * (T + 1) + T) * NX + jr];
  double s = rj ? -qfw2 * (tg - xT) : 0.0;
  if (task) {  // the task-space final cost (cost_functions.jl:16-24): ∇ℓ_f, ∇²ℓ_f on the q rows
    const size_t o = ((size_t)bc * (T + 1) + T) * NX;
    double g[2], H[3];
    chain_task_quad(task, (double)x[o], (double)x[o + 1], g, H);
    const double h0 = jr == 0 ? H[0] : H[1], h1 = jr == 0 ? H[1] : H[2];
    S = (rj && kap < NJ) ? (kap == 0 ? h0 : h1) : 0.0;
    s = rj ? (jr == 0 ? g[0] : g[1]) : 0.0;
  }

  const auto rJ = buffer_rsrc(const_cast<V*>(J) + (size_t)b0 * T * NR, (uint32_t)(nslot * T * NR * W));
  const uint32_t base = (uint32_t)(beta * T * NR * W);
  const uint32_t oA = base + (uint32_t)((rho * ND + kap) * W);
  const uint32_t oB = kap < NU ? base + (uint32_t)((rho * ND + NX + kap) * W) : DEAD;
  const uint32_t oT = rj ? base + (uint32_t)((NJAC + rho) * W) : DEAD;
  const uint32_t oU = ru ? base + (uint32_t)((NJAC + NX + rho) * W) : DEAD;
  const auto rK = buffer_rsrc(Kg + (size_t)b0 * T * NU * NX, (uint32_t)(nslot * T * NU * NX * W));
  const auto rD = buffer_rsrc(dg + (size_t)b0 * T * NU, (uint32_t)(nslot * T * NU * W));
  const uint32_t kv = (live && ru) ? (uint32_t)((beta * T * NU * NX + rho * NX + kap) * W) : DEAD;
  const uint32_t dv = (live && ru && kap == 0) ? (uint32_t)((beta * T * NU + rho) * W) : DEAD;
  const double Id = rho == kap ? 1.0 : 0.0;  // the identity block
  double* Hl = lds + beta * 16;

  constexpr int PF = CH_BW4_PF;
  // the ring holds the records' raw words: an fp32 record converted at the load would
  // make the step that issued it wait for it (the conversion consumes the load), which
  // defeats the prefetch — the conversion happens at the use, PF steps later
  using Raw = std::conditional_t<sizeof(V) == 4, uint32_t, double>;
  Raw rA[PF], rB[PF], rT[PF], rU[PF];
  auto ld = [&](uint32_t off, int t) -> Raw {
    if constexpr (sizeof(V) == 4)
      return __builtin_amdgcn_raw_buffer_load_b32(rJ, off, (uint32_t)(t * NR * W), 0);
    else
      return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rJ, off, (uint32_t)(t * NR * W), 0));
  };
  auto cv = [](Raw r) -> double {
    asm volatile("" : "+v"(r));  // the conversion stays at the use
    if constexpr (sizeof(V) == 4) return (double)__builtin_bit_cast(float, r);
    else return r;
  };
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    const int tk = T - 1 - k > 0 ? T - 1 - k : 0;
    rA[k] = ld(oA, tk); rB[k] = ld(oB, tk); rT[k] = ld(oT, tk); rU[k] = ld(oU, tk);
  }
  __builtin_amdgcn_s_waitcnt(0);
  double Kl = 0.0, dl = 0.0;
  auto step = [&](int t, int k) {
    const double A = cv(rA[k]), Bm = cv(rB[k]), th = cv(rT[k]), uu = cv(rU[k]);
    const int tn = t - PF > 0 ? t - PF : 0;
    rA[k] = ld(oA, tn); rB[k] = ld(oB, tn); rT[k] = ld(oT, tn); rU[k] = ld(oU, tn);
    const double lx = rj ? -qw2 * (tg - th) : 0.0;
    const double lu = rw2 * uu;
    const double Y0 = ch_mf(S, A, 0.0);
    const double Z = ch_mf(A, Y0, lxx);                           // lxx + AᵀSA
    const double G = ch_mf(Bm, Y0, 0.0);                          // BᵀSA
    const double gx = ch_mf(A, s, lx), gu = ch_mf(Bm, s, lu);     // lx + Aᵀs, lu + Bᵀs
    double K, d;
    if constexpr (NU == 2) {
      const double Y1 = ch_mf(S, Bm, 0.0);
      const double H = ch_mf(Bm, Y1, luu);                        // luu + BᵀSB
      Hl[rho * 4 + kap] = H;
      wave_lds_fence();
      const double h00 = Hl[0], h10 = Hl[4], h11 = Hl[5];
      wave_lds_fence();
      // (H + μI)⁻¹ of the 2×2 u block by its adjugate (H = luu + O(Δt²)BᵀSB)
      const double a00 = h00 + mu, a11 = h11 + mu;
      const double idet = rcp<2>(fma(a00, a11, -h10 * h10));
      const bool in2 = rho < 2 && kap < 2;
      const double Hi = !in2 ? 0.0 : (rho != kap ? -h10 : (rho == 0 ? a11 : a00)) * idet;
      K = ch_mfn(Hi, G, 0.0);
      d = ch_mfn(Hi, gu, 0.0);
    } else {
      // 1×1 H in every lane of the slot from B's column replicated over κ (a quad
      // broadcast): no LDS hand-off, and the gains are VALU products (ilqr_twolink.hip)
      const double Br = dpp_quad_bcast0(Bm);
      const double Y1 = ch_mf(S, Br, 0.0);                        // S·b, replicated
      const double H = ch_mf(Br, Y1, 2.0 * (double)P.rw[0]);      // luu + bᵀSb everywhere
      const double hi = rcp<2>(H + mu);
      K = -(hi * G);
      d = -(hi * gu);
      (void)Hl; (void)luu;
    }
    // wave-uniform soffset (a per-lane one makes each store a readfirstlane waterfall
    // loop); a DEAD voffset stays out of range whatever the step
    ch_st<V>(K, rK, kv, (uint32_t)(t * NU * NX * W));
    ch_st<V>(d, rD, dv, (uint32_t)(t * NU * W));
    const double Wk = fma(mu, K, -G), Wd = fma(mu, d, -gu);
    const double Sf = ch_mfn(K, Wk, Z);
    // Sfᵀ on the MFMA (ch_mf(Sf, I, 0), exact): its ≈50-cycle result instead of a
    // ds_bpermute round trip on the recursion's chain
    const double Sm = ch_mf(Sf, Id, 0.0);
    S = rho <= kap ? Sf : Sm;                                      // upper triangle, mirrored
    s = ch_mfn(K, Wd, gx);
    Kl = K; dl = d;
  };
  int t = T - 1;
  for (; t >= PF - 1; t -= PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) step(t - k, k);
  }
#pragma unroll
  for (int k = 0; k < PF - 1; ++k)
    if (t - k >= 0) step(t - k, k);
  const unsigned long long nb = __ballot(__builtin_isnan(Kl) || __builtin_isnan(dl));
  unsigned r = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) r |= (nb & ((0xFull << (4 * q)) * 0x0001000100010001ull)) ? (1u << q) : 0u;
  return r;
}

constexpr int CH_WG = 64;

// The chain constants go to LDS in the forward kernels: as a kernel argument they overflow
// the SGPR file (~210 SGPRs spilled to VGPR lanes at every use). WG threads copy and meet.
template <int WG, class PK>
__device__ __forceinline__ void chain_consts_to_lds(PK& Ps, const PK& P) {
  static_assert(sizeof(PK) % 4 == 0, "dword copy");
  for (int i = threadIdx.x; i < (int)(sizeof(PK) / 4); i += WG)
    reinterpret_cast<uint32_t*>(&Ps)[i] = reinterpret_cast<const uint32_t*>(&P)[i];
  __syncthreads();
}

// lanes per trajectory of the forward kernels: a 16-lane group (one DPP row) running
// the component-parallel Newton-Euler (chain_xdot_cv)
constexpr int CH_FW_LANES = 16;

// four trajectories per wave, four waves per workgroup (2-joint chains)
template <class V, int NU>
__global__ __launch_bounds__(256) void chain_backward4_kernel(ChainK<V, 2> P, int B, int T,
                                                              const V* __restrict__ x,
                                                              const V* __restrict__ J,
                                                              V* __restrict__ d, V* __restrict__ K,
                                                              int32_t* __restrict__ status, V mu,
                                                              const ChainTask* task) {
  __shared__ double lds[4 * 64];
  const int w = threadIdx.x >> 6;
  const int b0 = (blockIdx.x * 4 + w) * 4;
  if (b0 >= B) return;
  const unsigned nan = chain_backward4_wave<V, NU>(P, b0, B, 0xFu, T, x, J, d, K, (double)mu, lds + w * 64, task);
  const int l = threadIdx.x & 63;
  if (status && l < 4 && b0 + l < B) status[b0 + l] = ((nan >> l) & 1u) ? ILQR_TRAJ_NAN : ILQR_TRAJ_OK;
}

template <class V, int NJ, int NU>
__global__ __launch_bounds__(CH_WG) void chain_forward_kernel(
    ChainK<V, NJ> P, int B, int T, const V* __restrict__ x, const V* __restrict__ u,
    const V* __restrict__ xtraj, const V* __restrict__ d, const V* __restrict__ K,
    const V* __restrict__ prev_cost, V* __restrict__ xnew, V* __restrict__ unew,
    V* __restrict__ new_cost, int32_t* __restrict__ trials, int32_t* __restrict__ status,
    LSParams ls) {
  constexpr int NX = 2 * NJ;
  __shared__ ChainK<V, NJ> Ps;
  chain_consts_to_lds<CH_WG>(Ps, P);
  const int b = (blockIdx.x * CH_WG + threadIdx.x) / CH_FW_LANES;
  if (b >= B) return;  // the whole lane group
  const V pc = prev_cost ? prev_cost[b] : V(INFINITY);
  const ChainFwdOut<V> r =
      chain_forward_lane<V, NJ, NU, true>(Ps, b, T, x, u, xtraj, d, K, pc, xnew, unew, nullptr, ls);
  if ((threadIdx.x & 15) != 0) return;
  if (!r.accepted) {  // exhausted (the reference would loop forever): return the inputs
    for (int i = 0; i < (T + 1) * NX; ++i) xnew[(size_t)b * (T + 1) * NX + i] = x[(size_t)b * (T + 1) * NX + i];
    for (int i = 0; i < T * NU; ++i) unew[(size_t)b * T * NU + i] = u[(size_t)b * T * NU + i];
  }
  new_cost[b] = r.cost;
  if (trials) trials[b] = r.trials;
  if (status) status[b] = r.accepted ? ILQR_TRAJ_OK
                                     : (r.cost != r.cost ? ILQR_TRAJ_NAN : ILQR_TRAJ_LS_EXHAUSTED);
}

// fit iteration, backward part, 2-joint chains: slots whose status is not OK are
// computed on and never stored
template <class V, int NU>
__global__ __launch_bounds__(256) void chain_iter_backward4_kernel(ChainK<V, 2> P, int B, int T,
                                                                   ChainIter<V> a, const V* J, V mu,
                                                                   const ChainTask* task) {
  __shared__ double lds[4 * 64];
  const int w = threadIdx.x >> 6;
  const int b0 = (blockIdx.x * 4 + w) * 4;
  if (b0 >= B) return;
  unsigned active = 0;
  for (int q = 0; q < 4; ++q)
    if (b0 + q < B && a.status[b0 + q] == ILQR_TRAJ_OK) active |= 1u << q;
  if (active == 0) return;
  const unsigned nan =
      chain_backward4_wave<V, NU>(P, b0, B, active, T, a.x, J, a.d, a.K, (double)mu, lds + w * 64, task) &
      active;
  const int l = threadIdx.x & 63;
  if (l < 4 && ((nan >> l) & 1u)) {
    a.status[b0 + l] = ILQR_TRAJ_NAN;  // reference: AssertionError at backward_pass.jl:353
    if (a.res_parity) a.res_parity[b0 + l] = a.parity;
  }
}

template <class V, int NJ, int NU>
__global__ __launch_bounds__(CH_WG) void chain_iter_forward_kernel(ChainK<V, NJ> P, int B, int T,
                                                                   ChainIter<V> a, LSParams ls) {
  __shared__ ChainK<V, NJ> Ps;
  chain_consts_to_lds<CH_WG>(Ps, P);
  const int b = (blockIdx.x * CH_WG + threadIdx.x) / CH_FW_LANES;
  if (b >= B || a.status[b] != ILQR_TRAJ_OK) return;  // the whole lane group
  V du2 = V(0);
  const V pc = a.prev_cost ? a.prev_cost[b] : V(INFINITY);
  const ChainFwdOut<V> r = chain_forward_lane<V, NJ, NU, true>(Ps, b, T, a.x, a.u, a.xtraj, a.d,
                                                               a.K, pc, a.xnew, a.unew, &du2, ls);
  if ((threadIdx.x & 15) != 0) return;
  fwd_iter_finish(a, b, r.cost, r.accepted, r.trials, du2, ls.tol);
}

// ---------------------------------------------------------------------------
// Closed-form dynamics (ChainTrig): coefficient samples, the check against the
// recursion, and the forward kernels (one lane per trajectory: the closed form has
// nothing for a 16-lane group to split)
// ---------------------------------------------------------------------------
constexpr int CH_TRIG_SAMPLES = 15 + 18;  // M at 5 angles (3 entries), g on 3×3 (2 entries)
constexpr double two_pi = 6.283185307179586476925286766559;  // the sample grids' (device and host)
__global__ void chain_trig_sample_kernel(ChainK<double, 2> P, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double zero[2] = {0.0, 0.0}, e0[2] = {1.0, 0.0}, e1[2] = {0.0, 1.0};
  for (int k = 0; k < 5; ++k) {  // M(q₂ = 2πk/5); M does not depend on q₁
    double c[2] = {1.0, 0.0}, sn[2] = {0.0, 0.0};
    sincos(two_pi * k / 5.0, &sn[1], &c[1]);
    double m0[2], m1[2];
    rnea<false, false>(P, c, sn, zero, e0, m0);
    rnea<false, false>(P, c, sn, zero, e1, m1);
    out[3 * k] = m0[0];
    out[3 * k + 1] = 0.5 * (m1[0] + m0[1]);  // symmetric up to rounding
    out[3 * k + 2] = m1[1];
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {  // g(q₁ = 2πa/3, q₂ = 2πb/3)
      double c[2], sn[2], g[2];
      sincos(two_pi * a / 3.0, &sn[0], &c[0]);
      sincos(two_pi * b / 3.0, &sn[1], &c[1]);
      rnea<false, true>(P, c, sn, zero, zero, g);
      out[15 + 2 * (3 * a + b)] = g[0];
      out[15 + 2 * (3 * a + b) + 1] = g[1];
    }
}

// |f_trig − f_rnea| / max(1, |f_rnea|) at n pseudo-random states and torques (fp64)
__global__ void chain_trig_check_kernel(ChainK<double, 2> P, ChainTrig<double> Q, int n,
                                        double* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h = 0x9E3779B9u * (uint32_t)(i + 1);
  auto rnd = [&](double lo, double hi) {
    h ^= h << 13; h ^= h >> 17; h ^= h << 5;
    return lo + (hi - lo) * ((h & 0xFFFFFF) / 16777216.0);
  };
  double x[4] = {rnd(-4, 4), rnd(-4, 4), rnd(-6, 6), rnd(-6, 6)}, u[2] = {rnd(-3, 3), rnd(-3, 3)};
  double a[4], b[4];
  chain_xdot<2, 2>(P, x, u, a);
  chain_xdot_trig<2>(Q, x, u, b);
  double e = 0.0, m = 1.0;
  for (int k = 0; k < 4; ++k) {
    e = fmax(e, fabs(a[k] - b[k]));
    m = fmax(m, fabs(a[k]));
  }
  err[i] = e / m;
}

// L line-search candidates per trajectory (ilqr_fwd_group.h), W waves per workgroup
template <class V, int NU, int L, int W>
__global__ __launch_bounds__(64 * W) void chain_forward_trig_kernel(
    ChainTrig<V> P, int B, int T, const V* __restrict__ x, const V* __restrict__ u,
    const V* __restrict__ xtraj, const V* __restrict__ d, const V* __restrict__ K,
    const V* __restrict__ prev_cost, V* __restrict__ xnew, V* __restrict__ unew,
    V* __restrict__ new_cost, int32_t* __restrict__ trials, int32_t* __restrict__ status,
    LSParams ls) {
  constexpr int NX = 4;
  const int b = (blockIdx.x * 64 * W + threadIdx.x) / L;
  if (b >= B) return;
  const V pc = prev_cost ? prev_cost[b] : V(INFINITY);
  const ChainTrigModel<V, NU> m{P};
  const FgOut<V> r = fwd_group<ChainTrigModel<V, NU>, L>(m, b, B, T, x, u, xtraj, d, K, pc, xnew, unew, ls);
  if (!r.owner) return;
  if (!r.accepted) {  // exhausted (the reference would loop forever): return the inputs
    for (int i = 0; i < (T + 1) * NX; ++i) xnew[(size_t)b * (T + 1) * NX + i] = x[(size_t)b * (T + 1) * NX + i];
    for (int i = 0; i < T * NU; ++i) unew[(size_t)b * T * NU + i] = u[(size_t)b * T * NU + i];
  }
  new_cost[b] = r.cost;
  if (trials) trials[b] = r.trials;
  if (status) status[b] = r.accepted ? ILQR_TRAJ_OK
                                     : (r.cost != r.cost ? ILQR_TRAJ_NAN : ILQR_TRAJ_LS_EXHAUSTED);
}

template <class V, int NU, int L, int W>
__global__ __launch_bounds__(64 * W) void chain_iter_forward_trig_kernel(ChainTrig<V> P, int B, int T,
                                                                         ChainIter<V> a, LSParams ls) {
  const int b = (blockIdx.x * 64 * W + threadIdx.x) / L;
  if (b >= B || a.status[b] != ILQR_TRAJ_OK) return;
  const V pc = a.prev_cost ? a.prev_cost[b] : V(INFINITY);
  const ChainTrigModel<V, NU> m{P};
  const FgOut<V> r = fwd_group<ChainTrigModel<V, NU>, L>(m, b, B, T, a.x, a.u, a.xtraj, a.d, a.K, pc, a.xnew,
                                                          a.unew, ls, a.res_parity == nullptr);
  if (!r.owner) return;
  fwd_iter_finish(a, b, r.cost, r.accepted, r.trials, r.du2, ls.tol);
}

// ---------------------------------------------------------------------------
// Chains on the tiles path (NJ = NU = 4..7 joints, every joint driven: the 6-DoF arm, a
// 7-DoF manipulator; nx = 2·NJ, fp64). The Riccati recursion is a tiles kernel
// (launch_tiles_backward, ilqr_tiles.hip: the narrow one for 8 × 4, the wide one beyond), so
// the linearisation and the costs are written as the tiles it reads — A (B,T,nx,nx),
// B (B,T,nx,nu), lx, lu, lxx, luu, lfx, lfxx — and the forward runs a 32-lane group per
// trajectory (chain_xdot_cv32).
// ---------------------------------------------------------------------------
// chain_linearize_kernel's lane map (one lane per (b, t, direction)) and arithmetic; lane
// kd stores column kd of A_t (kd < NX) or column kd − NX of B_t
constexpr int CHAIN_TILES_FD_WAVES = 1, CHAIN_TILES_DUAL_WAVES = 1;
template <int NJ, int NU, int LIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LIN == ILQR_LINEARIZE_CENTRAL_FD ? CHAIN_TILES_FD_WAVES : CHAIN_TILES_DUAL_WAVES))) void chain_linearize_tiles_kernel(ChainK<double, NJ> P, int B, int T,
                                                                    const double* __restrict__ x,
                                                                    const double* __restrict__ u,
                                                                    const int32_t* __restrict__ status,
                                                                    double* __restrict__ A,
                                                                    double* __restrict__ Bm) {
  using V = double;
  constexpr int NX = 2 * NJ, ND = NX + NU;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * T * ND) return;
  const size_t bt = g / ND;
  const int kd = (int)(g - bt * ND);
  const int b = (int)(bt / T), t = (int)(bt - (size_t)b * T);
  if (status && status[b] != ILQR_TRAJ_OK) return;
  const V* xb = x + ((size_t)b * (T + 1) + t) * NX;
  const V* ub = u + bt * NU;
  V z[ND], col[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) z[k] = xb[k];
#pragma unroll
  for (int k = 0; k < NU; ++k) z[NX + k] = ub[k];
  if constexpr (LIN == ILQR_LINEARIZE_DUAL) {
    using D = DualT<1, V>;
    D xs[NX], us[NU], o[NX];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      D v(z[k]);
      v.d[0] = (k == kd) ? V(1) : V(0);
      if (k < NX) xs[k] = v; else us[k - NX] = v;
    }
    chain_rk4<NJ, NU>(P, xs, us, o);
#pragma unroll
    for (int i = 0; i < NX; ++i) col[i] = o[i].d[0];
  } else {
    // central differences, step h = ε^(1/3)·max(1, |z_k|), divided by the step actually taken
    const V cbe = V(6.0554544523933395e-6);
    V zk = z[0];
#pragma unroll
    for (int j = 1; j < ND; ++j)
      if (j == kd) zk = z[j];
    const V h = cbe * fmax(V(1), fabs(zk));
    const V zp = zk + h, zm = zk - h;
    V xp[NX], up[NU], xm[NX], um[NU], fp[NX], fm[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      xp[j] = j == kd ? zp : z[j];
      xm[j] = j == kd ? zm : z[j];
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      up[j] = NX + j == kd ? zp : z[NX + j];
      um[j] = NX + j == kd ? zm : z[NX + j];
    }
    chain_rk4<NJ, NU>(P, xp, up, fp);
    chain_rk4<NJ, NU>(P, xm, um, fm);
    const V inv = V(1) / (zp - zm);
#pragma unroll
    for (int i = 0; i < NX; ++i) col[i] = (fp[i] - fm[i]) * inv;
  }
  V* out = kd < NX ? A + bt * NX * NX + kd : Bm + bt * NX * NU + (kd - NX);
  const int ld = kd < NX ? NX : NU;
#pragma unroll
  for (int i = 0; i < NX; ++i) out[i * ld] = col[i];
}

// ILQR_LINEARIZE_ANALYTIC: the exact Jacobians without differentiating M or the solve. For
// q̈ = M(q)⁻¹(τ − b(q, q̇)), ID(q, q̇, q̈) = M q̈ + b is the Newton-Euler pass and
//   δq̈ = M⁻¹(δτ − δ[ID(q, q̇, q̈)]),  q̈ held fixed,
// so a direction costs one tangent pass (rnea<true, true> in DualT<1>) and one solve with the
// stage's M per RK4 stage, and the stage's primal (M, b, q̈) is the same for the 3·NJ directions
// of a point (DESIGN.md "The analytic linearisation").
//
// Lane map: a point (b, t) is ND = 3·NJ consecutive lanes of one wave, PPW = 64 / ND points
// per wave (the wave's last 64 − PPW·ND lanes idle along on its first point and store
// nothing); lane kd of a point carries direction kd of [δx | δu] and stores column kd of
// [A | B] as chain_linearize_tiles_kernel does. Per stage, lane kd ≤ NJ of the point also runs
// pass kd of the primal — 0: the bias (q̇, 0, gravity), k + 1: column k of M (0, e_k, no
// gravity), one uniform rnea<true, true> with per-lane arguments as in the forward group — and
// the NJ + 1 results reach the point's lanes through a wave-private LDS region. Every lane
// then eliminates M itself (chain_xdot's elimination), for q̈ and again for δq̈: the second
// solve reads M from the region again, so keeping the factor over the tangent pass or redoing
// it is the compiler's choice (it keeps the multipliers: six reciprocals per stage at six joints).
// No lane leaves early and there is no workgroup barrier: a lane past the last point or on
// a stopped trajectory computes on a clamped point and skips the store.
// One wave per SIMD: the tangent pass keeps R, fn and ff as duals (180 doubles at six joints;
// profiles/chain_analytic/resource_usage.txt). The chain constants stay kernel arguments:
// read from LDS instead (chain_consts_to_lds) the SGPR-spill v_readlanes go (10,004 → 8,149
// instructions per stage at six joints) but the constants then compete for VGPRs, scratch
// doubles to 1.4 KB per lane and the kernel is slower at five to seven joints (8.67 → 14.67 ms
// at six; profiles/chain_analytic/lds_constants.txt).
constexpr int CHAIN_ANALYTIC_WAVES = 1;
// o = M⁻¹ r, M's column k at m[(k + 1)·NJ ..] (the exchange region; m[0 .. NJ) is the bias)
template <int NJ>
__device__ __forceinline__ void chain_analytic_solve(const double* m, double (&r)[NJ], double (&o)[NJ]) {
  double M[NJ][NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k)
#pragma unroll
    for (int i = 0; i < NJ; ++i) M[i][k] = m[(k + 1) * NJ + i];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const double inv = crecip(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < NJ; ++i) {
      const double l = M[i][k] * inv;
#pragma unroll
      for (int j = k + 1; j < NJ; ++j) M[i][j] = M[i][j] - l * M[k][j];
      r[i] = r[i] - l * r[k];
    }
  }
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    double acc = r[i];
#pragma unroll
    for (int j = i + 1; j < NJ; ++j) acc = acc - M[i][j] * o[j];
    o[i] = acc * crecip(M[i][i]);
  }
}

template <int NJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CHAIN_ANALYTIC_WAVES))) void chain_linearize_analytic_kernel(
    ChainK<double, NJ> P, int B, int T, const double* __restrict__ x, const double* __restrict__ u,
    const int32_t* __restrict__ status, double* __restrict__ A, double* __restrict__ Bm) {
  using V = double;
  using D = DualT<1, V>;
  constexpr int NU = NJ, NX = 2 * NJ, ND = NX + NU, PPW = 64 / ND, NE = (NJ + 1) * NJ;
  static_assert(3 * NJ <= 64, "a point's directions are lanes of one wave");
  __shared__ V xch[4][PPW][NE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pw_ = lane / ND;
  const bool spare = pw_ >= PPW;  // the wave's lanes past its last point
  const int pw = spare ? 0 : pw_;
  const int kd = lane - pw_ * ND;
  const size_t npt = (size_t)B * T;
  size_t bt = ((size_t)blockIdx.x * 4 + wave) * PPW + pw;
  bool store = !spare && bt < npt;
  if (bt >= npt) bt = npt - 1;  // reads stay in range
  const int b = (int)(bt / T), t = (int)(bt - (size_t)b * T);
  if (status && status[b] != ILQR_TRAJ_OK) store = false;
  const V* xb = x + ((size_t)b * (T + 1) + t) * NX;
  const V* ub = u + bt * NU;
  V* reg = xch[wave][pw];
  const bool pass = !spare && kd <= NJ;  // this lane's primal pass is one of the point's NJ + 1
  V xs[NX], us[NU], kp[NX], dkp[NX], acc[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    xs[i] = xb[i];
    kp[i] = V(0);
    dkp[i] = V(0);
    acc[i] = V(0);
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) us[i] = ub[i];
  // the stages as one loop: y_s = x + a_s k_{s−1} with a = 0, ½, ½, 1 (k₀ = 0) and the sum
  // ((δk₁ + 2δk₂) + 2δk₃) + δk₄ accumulated in chain_rk4's association
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    const V a = s == 0 ? V(0) : s == 3 ? V(1) : V(0.5);
    const V wgt = (s == 1 || s == 2) ? V(2) : V(1);
    V y[NX], dy[NX], c[NJ], sn[NJ];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      y[i] = xs[i] + a * kp[i];
      dy[i] = (i == kd ? V(1) : V(0)) + a * dkp[i];
    }
#pragma unroll
    for (int i = 0; i < NJ; ++i) scs(y[i], sn[i], c[i]);
    {  // the primal: pass kd of the point
      V qd[NJ], qdd[NJ], tau[NJ];
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        qd[i] = kd == 0 ? y[NJ + i] : V(0);
        qdd[i] = kd == i + 1 ? V(1) : V(0);
      }
      rnea<true, true>(P, c, sn, qd, qdd, tau, kd == 0 ? V(1) : V(0));
      wave_lds_fence();  // the previous stage's reads of the region are done
      if (pass) {
#pragma unroll
        for (int i = 0; i < NJ; ++i) reg[kd * NJ + i] = tau[i];
      }
      wave_lds_fence();
    }
    V qdd[NJ], r[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) r[i] = us[i] - reg[i];
    chain_analytic_solve<NJ>(reg, r, qdd);
    // δ[ID(q, q̇, q̈)] along this lane's direction
    V dqdd[NJ];
    {
      D cD[NJ], sD[NJ], qdD[NJ], qddD[NJ], tauD[NJ];
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        cD[i].v = c[i];
        cD[i].d[0] = -sn[i] * dy[i];
        sD[i].v = sn[i];
        sD[i].d[0] = c[i] * dy[i];
        qdD[i].v = y[NJ + i];
        qdD[i].d[0] = dy[NJ + i];
        qddD[i] = D(qdd[i]);
      }
      rnea<true, true>(P, cD, sD, qdD, qddD, tauD);
#pragma unroll
      for (int i = 0; i < NJ; ++i) r[i] = (NX + i == kd ? V(1) : V(0)) - tauD[i].d[0];
    }
    chain_analytic_solve<NJ>(reg, r, dqdd);
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      kp[i] = P.dt * y[NJ + i];
      kp[NJ + i] = P.dt * qdd[i];
      dkp[i] = P.dt * dy[NJ + i];
      dkp[NJ + i] = P.dt * dqdd[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = acc[i] + wgt * dkp[i];
  }
  if (!store) return;
  V* out = kd < NX ? A + bt * NX * NX + kd : Bm + bt * NX * NU + (kd - NX);
  const int ld = kd < NX ? NX : NU;
#pragma unroll
  for (int i = 0; i < NX; ++i) out[i * ld] = (i == kd ? V(1) : V(0)) + (V(1) / V(6)) * acc[i];
}

// the joint-space cost (RBD_helper_functions.jl:85-116) of an NJ-joint chain
template <int NJ>
struct ChainCostK {
  double tgt[NJ], qw[NJ], rw[NJ], qfw[NJ];
};

// A goal per trajectory (ilqr_chain_set_joint_targets: NJ doubles a row, θ*;
// ilqr_chain_set_task_targets: 3 doubles a row, final_target): the handle's copy of the rows.
// Every kernel that reads a goal takes it as a trailing pack beside its constants — empty for
// a handle without rows, whose instantiations, kernel arguments and code stay what they were
// (the TaskK pack of the forward kernels below) — and, with it, reads row b where it read
// the constant: the same expression in the same order, another source.
struct ChainGoalRows {
  const double* rows;
};
__device__ __forceinline__ const double* goal_rows(const ChainGoalRows& g) { return g.rows; }

// The cost tiles that change with (x, u), the terms chain_backward4_wave forms for two joints
// (immediate_cost_quadratization :81-109, final_cost_quadratization :134-153):
// lx = −2qw(θ* − θ) on the joint rows, lu = 2rw·u, lfx = −2qfw(θ* − θ_N).
// One lane per element: (b, t ≤ T, e < NX + NU), t = T the terminal row.
// Goal: none (θ* = C.tgt) or ChainGoalRows (θ* = row b).
template <int NJ, int NU, class... Goal>
__global__ __launch_bounds__(256) void chain_cost_tiles_kernel(ChainCostK<NJ> C, Goal... G, int B, int T,
                                                               const double* __restrict__ x,
                                                               const double* __restrict__ u,
                                                               const int32_t* __restrict__ status,
                                                               double* __restrict__ lx, double* __restrict__ lu,
                                                               double* __restrict__ lfx) {
  constexpr int NX = 2 * NJ, NE = NX + NU;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * (T + 1) * NE) return;
  const size_t bt = g / NE;
  const int e = (int)(g - bt * NE);
  const int b = (int)(bt / (T + 1)), t = (int)(bt - (size_t)b * (T + 1));
  if (status && status[b] != ILQR_TRAJ_OK) return;
  const int j = e < NJ ? e : (e >= NX ? e - NX : 0);  // the joint / input of this element
  double tgt = C.tgt[0], qw = C.qw[0], rw = C.rw[0], qfw = C.qfw[0];
#pragma unroll
  for (int i = 1; i < NJ; ++i)
    if (i == j) { tgt = C.tgt[i]; qw = C.qw[i]; rw = C.rw[i]; qfw = C.qfw[i]; }
  static_assert((std::is_same_v<Goal, ChainGoalRows> && ...) && sizeof...(Goal) <= 1, "Goal: none or ChainGoalRows");
  if constexpr (sizeof...(Goal) == 1)
    if (e < NJ) tgt = goal_rows(G...)[(size_t)b * NJ + e];
  if (e < NX) {
    const double xe = x[((size_t)b * (T + 1) + t) * NX + e];
    if (t == T) lfx[(size_t)b * NX + e] = e < NJ ? -2.0 * qfw * (tgt - xe) : 0.0;
    else lx[((size_t)b * T + t) * NX + e] = e < NJ ? -2.0 * qw * (tgt - xe) : 0.0;
  } else if (t < T) {
    const size_t i = ((size_t)b * T + t) * NU + (e - NX);
    lu[i] = 2.0 * rw * u[i];
  }
}

// The Hessian tiles lxx = diag(2qw, 0), luu = diag(2rw), lfxx = diag(2qfw, 0): they depend
// on neither the state nor the step, so they are written when the handle is created and
// when its cost mode changes (a task mode: q = qf = 0, r = 1, and lfxx rewritten by every
// backward). One lane per (b, t ≤ T, element of the larger tile).
template <int NJ, int NU>
__global__ __launch_bounds__(256) void chain_cost_hessians_kernel(ChainCostK<NJ> C, int B, int T,
                                                                  double* __restrict__ lxx,
                                                                  double* __restrict__ luu,
                                                                  double* __restrict__ lfxx) {
  constexpr int NX = 2 * NJ;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)B * (T + 1) * NX * NX) return;
  const size_t bt = g / (NX * NX);
  const int e = (int)(g - bt * (NX * NX));
  const int b = (int)(bt / (T + 1)), t = (int)(bt - (size_t)b * (T + 1));
  const int r = e / NX, c = e - r * NX;
  double qw = 0.0, rw = 0.0, qfw = 0.0;
#pragma unroll
  for (int i = 0; i < NJ; ++i)
    if (i == r) { qw = C.qw[i]; qfw = C.qfw[i]; }
  const int ru = e / NU, cu = e - ru * NU;
#pragma unroll
  for (int i = 0; i < NU; ++i)
    if (i == ru) rw = C.rw[i];
  if (t == T) {
    lfxx[(size_t)b * NX * NX + e] = (r == c && r < NJ) ? 2.0 * qfw : 0.0;
  } else {
    const size_t s = (size_t)b * T + t;
    lxx[s * NX * NX + e] = (r == c && r < NJ) ? 2.0 * qw : 0.0;
    if (e < NU * NU) luu[s * NU * NU + e] = ru == cu ? 2.0 * rw : 0.0;
  }
}

// ---------------------------------------------------------------------------
// cost_functions.jl's task-space costs on the tiles path (ilqr_chain_set_task_costs): the
// point's kinematics composed at every evaluation. The sampled polynomial of the 2-joint
// closed form (ChainTask) would carry 3^NJ coefficients here.
// ---------------------------------------------------------------------------
struct ChainTaskK {
  double pt[3];     // the point in body `body`'s frame
  double t[3];      // final_target
  double w;         // weight
  int32_t body;     // −1 (the fixed base) .. NJ − 1
  int32_t literal;  // the reference's reading: p_z against every target component
};

// (transform_to_root(state, body) * point).v: x_parent = p_i + R0_i·Rot(a_i, q_i)·x_child
// from `body` down, in chain_point_position's / oracle.cost_functions.point_position's
// operation order and without contraction, so the value differs from theirs by the
// rounding of sin and cos only. Uniform in the lane: no lane-dependent order.
template <int NJ>
__device__ __forceinline__ void chain_point_fk(const ChainK<double, NJ>& P, const ChainTaskK& C,
                                               const double (&q)[NJ], double (&p)[3]) {
#pragma clang fp contract(off)
  double w[3] = {C.pt[0], C.pt[1], C.pt[2]};
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    if (i > C.body) continue;
    double s, c;
    vsincos(q[i], s, c);
    const double a0 = P.ax[i][0], a1 = P.ax[i][1], a2 = P.ax[i][2];
    const double axw[3] = {a1 * w[2] - a2 * w[1], a2 * w[0] - a0 * w[2], a0 * w[1] - a1 * w[0]};
    const double adw = a0 * w[0] + a1 * w[1] + a2 * w[2];
    const double k = (1.0 - c) * adw;
    double r[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) r[e] = c * w[e] + s * axw[e] + k * P.ax[i][e];
#pragma unroll
    for (int e = 0; e < 3; ++e)
      w[e] = P.p[i][e] + (P.R0[i][3 * e] * r[0] + P.R0[i][3 * e + 1] * r[1] + P.R0[i][3 * e + 2] * r[2]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) p[e] = w[e];
}

// ℓ_f = weight · ((e₁² + e₂²) + e₃²), eₖ = p_k − t_k (p_z for every k in the reference's
// reading), the oracle's summation order (cost_functions.jl:21-23)
__device__ __forceinline__ double chain_task_value(const ChainTaskK& C, const double (&p)[3]) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double e = (C.literal ? p[2] : p[k]) - C.t[k];
    acc = acc + e * e;
  }
  return C.w * acc;
}

// simple_immediate_cost: Σ uᵢ², `acc + u*u` in index order (cost_functions.jl:45-51)
template <int NU>
__device__ __forceinline__ double chain_task_stage(const double (&u)[NU]) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < NU; ++a) acc = acc + u[a] * u[a];
  return acc;
}

// final_cost_quadratization (backward_pass.jl:134-153) of the task cost at one state:
// ℓ_f, ∇ℓ_f = 2w Σₖ eₖ∇pₖ and the upper triangle i ≤ j of ∇²ℓ_f = 2w Σₖ (∇pₖ∇pₖᵀ + eₖ∇²pₖ)
// on the joint block. The derivatives are analytic in geometric form: with âᵢ, oᵢ the
// root-frame axis and origin of joint i (one root-to-tip pass of the joint transforms),
// ∂p/∂qᵢ = âᵢ × (p − oᵢ) and ∂²p/∂qᵢ∂qⱼ = âᵢ × ∂p/∂qⱼ for i ≤ j ≤ body, zero beyond `body`.
template <int NJ>
__device__ void chain_task_quad_fk(const ChainK<double, NJ>& P, const ChainTaskK& C, const double (&q)[NJ],
                                 double& cost, double (&g)[NJ], double (&H)[NJ][NJ]) {
  double p[3];
  chain_point_fk<NJ>(P, C, q, p);
  cost = chain_task_value(C, p);
  double Rw[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, o[3] = {0.0, 0.0, 0.0};
  double ah[NJ][3], J[NJ][3];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    if (i > C.body) {
#pragma unroll
      for (int e = 0; e < 3; ++e) ah[i][e] = J[i][e] = 0.0;
      continue;
    }
    double s, c, R[9], Rn[9], on[3];
    vsincos(q[i], s, c);
    joint_rot(P, i, c, s, R);
    to_parent(Rw, P.p[i], on);  // oᵢ = o_parent + R_parent pᵢ
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] += on[e];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        Rn[3 * r + k] = Rw[3 * r] * R[k] + Rw[3 * r + 1] * R[3 + k] + Rw[3 * r + 2] * R[6 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = Rn[k];
    to_parent(Rw, P.ax[i], ah[i]);  // âᵢ (the axis is fixed in the joint's own frame)
    const double r[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
    cross3(ah[i], r, J[i]);
  }
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = (C.literal ? p[2] : p[k]) - C.t[k];
  const double w2 = 2.0 * C.w;
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    double gi = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) gi += e[k] * (C.literal ? J[i][2] : J[i][k]);
    g[i] = w2 * gi;
#pragma unroll
    for (int j = i; j < NJ; ++j) {
      double d2[3];
      cross3(ah[i], J[j], d2);  // ∂²p/∂qᵢ∂qⱼ, i ≤ j
      double hij = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int m = C.literal ? 2 : k;
        hij += J[i][m] * J[j][m] + e[k] * d2[m];
      }
      H[i][j] = w2 * hij;
    }
  }
}

// The quadratization at n states x[s·xstride .. +2NJ), one lane per state:
//  * the terminal tiles of a task mode (xstride = (T + 1)·NX, x offset to x_N by the
//    caller): lfx and lfxx, the latter exactly symmetric (i ≤ j computed, mirrored: the
//    tiles recursion takes it as S_N), velocity rows and columns exactly 0; trajectories
//    whose status is not OK are skipped like chain_cost_tiles_kernel's;
//  * ilqr_chain_final_cost_quadratize (xstride = NX), any output null; in the joint mode
//    (joint = 1) the handle's joint-space final cost Σ qfwᵢ(θ*ᵢ − θᵢ)² instead.
// Goal: none, or ChainGoalRows — the goal of state s is row s (NJ doubles with joint = 1,
// 3 otherwise; the caller has n ≤ the rows it holds).
template <int NJ, class... Goal>
__global__ __launch_bounds__(64) void chain_task_quad_kernel(ChainK<double, NJ> P, ChainTaskK C, Goal... G, int joint,
                                                             int n, const double* __restrict__ x, size_t xstride,
                                                             const int32_t* __restrict__ status,
                                                             double* __restrict__ cost, double* __restrict__ grad,
                                                             double* __restrict__ hess) {
  constexpr int NX = 2 * NJ;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  if (status && status[b] != ILQR_TRAJ_OK) return;
  const double* xb = x + (size_t)b * xstride;
  double q[NJ], c, g[NJ], H[NJ][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) q[i] = xb[i];
  static_assert((std::is_same_v<Goal, ChainGoalRows> && ...) && sizeof...(Goal) <= 1, "Goal: none or ChainGoalRows");
  constexpr bool ROWS = sizeof...(Goal) == 1;
  if (joint) {
    c = 0.0;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      double tg = P.tgt[i];
      if constexpr (ROWS) tg = goal_rows(G...)[(size_t)b * NJ + i];
      const double e = tg - q[i];
      c = fma(P.qfw[i] * e, e, c);
      g[i] = -2.0 * P.qfw[i] * e;
#pragma unroll
      for (int j = i; j < NJ; ++j) H[i][j] = i == j ? 2.0 * P.qfw[i] : 0.0;
    }
  } else if constexpr (ROWS) {
    ChainTaskK Cb = C;
#pragma unroll
    for (int k = 0; k < 3; ++k) Cb.t[k] = goal_rows(G...)[(size_t)b * 3 + k];
    chain_task_quad_fk<NJ>(P, Cb, q, c, g, H);
  } else {
    chain_task_quad_fk<NJ>(P, C, q, c, g, H);
  }
  if (cost) cost[b] = c;
  if (grad) {
    double* go = grad + (size_t)b * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) go[i] = i < NJ ? g[i] : 0.0;
  }
  if (hess) {
    double* ho = hess + (size_t)b * NX * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        ho[i * NX + j] = hi < NJ ? H[lo][hi] : 0.0;
      }
  }
}

// Forward rollout + α-halving line search of a chain on the tiles path: chain_forward_lane's
// arithmetic in its order, every lane of a 32-lane group carrying the same x̄, ū, cost and
// Σδu² (the dynamics split over the group: chain_xdot_cv32).
//  * Step inputs (K_t NU×NX, x_t, x_traj_t's joint rows, u_t, δu_t: N_IN = NU·NX + NX + NJ +
//    2·NU doubles — 52, 75, 102, 133 for 4..7 joints) are loaded one step ahead, lane l the
//    words l, l + 32, … of the step's record, and handed to the group through LDS at the
//    top of the step (as registers per lane and step in flight they would not fit);
//  * the staging is sized per instantiation: ⌈N_IN / 32⌉ words per lane (2, 3, 4, 5) and a
//    stage of 32 × that many doubles (64, 96, 128, 160) per group;
//  * x̄_t and ū_t are stored by lanes 0..NX − 1 and NX..NX + NU − 1 (one coalesced store each).
constexpr int CH32_LANES = 32;
template <int NJ, int NU>
struct ChainStage {
  static constexpr int N_IN = NU * 2 * NJ + 2 * NJ + NJ + 2 * NU;  // a step's record
  static constexpr int WORDS = (N_IN + CH32_LANES - 1) / CH32_LANES;  // per lane
  static constexpr int SIZE = CH32_LANES * WORDS;                     // doubles per group
};
static_assert(ChainStage<6, 6>::WORDS == 4 && ChainStage<6, 6>::SIZE == 128, "six joints: four words per lane");
static_assert(ChainStage<7, 7>::WORDS == 5 && ChainStage<7, 7>::SIZE == 160, "seven joints: five words per lane");
// TASK: the costs of a task mode (ℓ = Σū², ℓ_f the task cost C of x̄_N, every lane of the
// group evaluating it on its own copy of x̄_N by the same code: the same bits in all 32) in
// place of the joint-space ones, chosen at compile time so that the joint-cost
// instantiations keep their instruction streams.
// ROWS: the goal of trajectory b is row b of `goal` (NJ doubles, θ*; 3 with TASK, final_target)
// in place of P.tgt / C.t, likewise a compile-time choice. The row rides in the stage's unused
// tail, which every lane count leaves (12, 21, 20 and 27 words for 4..7 joints): the lanes
// whose words fall past the record re-read K's first word at every step anyway, so with ROWS
// the first NG of those words read the row instead (stride 0) and the hand-off delivers it
// to the group at stage[N_IN ..) — no register beyond what the shared-goal code holds, which
// at seven joints already fills both register files.
template <int NJ, int NU, bool TASK = false, bool ROWS = false, class... Goal>
__device__ ChainFwdOut<double> chain_forward_group32(const ChainK<double, NJ>& P, double* __restrict__ stage,
                                                     int b, int T, const double* __restrict__ x,
                                                     const double* __restrict__ u,
                                                     const double* __restrict__ xtraj,
                                                     const double* __restrict__ dg,
                                                     const double* __restrict__ Kg, double prev_cost,
                                                     double* __restrict__ xnew, double* __restrict__ unew,
                                                     double* du2_out, const LSParams& ls,
                                                     const ChainTaskK& C = ChainTaskK{}, const Goal&... G) {
  using V = double;
  static_assert((std::is_same_v<Goal, ChainGoalRows> && ...) && sizeof...(Goal) == (ROWS ? 1 : 0),
                "Goal: ChainGoalRows with ROWS, else none (the shared-goal instantiations keep their signature)");
  constexpr int NX = 2 * NJ, NK = NU * NX;
  constexpr int O_X = NK, O_XT = O_X + NX, O_U = O_XT + NJ, O_D = O_U + NU, N_IN = O_D + NU;
  constexpr int NW = ChainStage<NJ, NU>::WORDS;
  static_assert(N_IN == ChainStage<NJ, NU>::N_IN && N_IN <= ChainStage<NJ, NU>::SIZE && NX + NU <= CH32_LANES,
                "a step's inputs in NW words per lane, x̄ and ū stored by one lane each");
  constexpr int NG = ROWS ? (TASK ? 3 : NJ) : 0, O_G = N_IN;  // the goal row in the stage's tail
  static_assert(N_IN + NG <= ChainStage<NJ, NU>::SIZE, "the goal row fits the stage's unused tail");
  const int l32 = threadIdx.x & (CH32_LANES - 1);
  const V* xb0 = x + (size_t)b * (T + 1) * NX;
  const V* ub0 = u + (size_t)b * T * NU;
  const V* xt0 = (xtraj ? xtraj : x) + (size_t)b * (T + 1) * NX;
  const V xtw = xtraj ? V(1) : V(0);  // x_traj = NULL means zeros (forward_pass.jl:151)
  const V* d0 = dg + (size_t)b * T * NU;
  const V* K0 = Kg + (size_t)b * T * NK;
  V* xo = xnew + (size_t)b * (T + 1) * NX;
  V* uo = unew + (size_t)b * T * NU;
  // this lane's NW words of a step's record: source and stride per step (a word past the
  // record re-reads K's first word and lands in the stage's unused tail)
  const V* src[NW];
  int str[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int e = l32 + CH32_LANES * k;
    src[k] = K0, str[k] = 0;
    if (e < O_X) { src[k] = K0 + e; str[k] = NK; }
    else if (e < O_XT) { src[k] = xb0 + (e - O_X); str[k] = NX; }
    else if (e < O_U) { src[k] = xt0 + (e - O_XT); str[k] = NX; }
    else if (e < O_D) { src[k] = ub0 + (e - O_U); str[k] = NU; }
    else if (e < N_IN) { src[k] = d0 + (e - O_D); str[k] = NU; }
    else if constexpr (ROWS) {  // stride 0: the row at every step
      if (e < O_G + NG) src[k] = goal_rows(G...) + (size_t)b * NG + (e - O_G);
    }
  }
  V alpha = V(ls.alpha0);
  ChainFwdOut<V> out{V(0), 0, 0};
  V du2 = V(0);
  for (int trial = 1; trial <= ls.max_trials; ++trial) {
    V xb[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xb[i] = xb0[i];  // x̄₁ = x₁ (:65)
    V cost = V(0);
    du2 = V(0);
    V in[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) in[k] = src[k][0];
    for (int t = 0; t < T; ++t) {
      wave_lds_fence();  // the previous step's reads are done
#pragma unroll
      for (int k = 0; k < NW; ++k) stage[l32 + CH32_LANES * k] = in[k];
      wave_lds_fence();
      {
        const size_t tn = t + 1 < T ? t + 1 : t;  // step t + 1's words, in flight during step t
#pragma unroll
        for (int k = 0; k < NW; ++k) in[k] = src[k][tn * str[k]];
      }
      V dx[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) dx[i] = xb[i] - stage[O_X + i];  // δx (:72)
      V ubar[NU];
#pragma unroll
      for (int a = 0; a < NU; ++a) {  // ūₖ = uₖ + α δuₖ + Kₖ δx (:73)
        V kdx = V(0);
#pragma unroll
        for (int i = 0; i < NX; ++i) kdx = fma(stage[a * NX + i], dx[i], kdx);
        const V uk = stage[O_U + a];
        ubar[a] = fma(alpha, stage[O_D + a], uk) + kdx;
        const V e = ubar[a] - uk;
        du2 = fma(e, e, du2);
      }
      // ℓ(x̄ₖ − x_trajₖ, ūₖ) (:187-190; RBD_helper_functions.jl:85-99 on the joints)
      V lk = V(0);
      if constexpr (TASK) {
        lk = chain_task_stage<NU>(ubar);  // ignores x and x_traj (cost_functions.jl:45-51)
      } else {
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
          if constexpr (ROWS) {
            const V e = stage[O_G + i] - fma(-xtw, stage[O_XT + i], xb[i]);
            lk = fma(P.qw[i] * e, e, lk);
          } else {
            const V e = P.tgt[i] - fma(-xtw, stage[O_XT + i], xb[i]);
            lk = fma(P.qw[i] * e, e, lk);
          }
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) lk = fma(P.rw[a] * ubar[a], ubar[a], lk);
      }
      cost += lk;
      {
        V w = xb[0];
#pragma unroll
        for (int i = 1; i < NX; ++i)
          if (l32 == i) w = xb[i];
#pragma unroll
        for (int a = 0; a < NU; ++a)
          if (l32 == NX + a) w = ubar[a];
        if (l32 < NX) xo[(size_t)t * NX + l32] = w;
        else if (l32 < NX + NU) uo[(size_t)t * NU + (l32 - NX)] = w;
      }
      V xn[NX];
      chain_rk4_cv32<NJ, NU>(P, xb, ubar, xn);  // x̄ₖ₊₁ = f(x̄ₖ, ūₖ) (:74)
#pragma unroll
      for (int i = 0; i < NX; ++i) xb[i] = xn[i];
    }
    {
      V w = xb[0];
#pragma unroll
      for (int i = 1; i < NX; ++i)
        if (l32 == i) w = xb[i];
      if (l32 < NX) xo[(size_t)T * NX + l32] = w;
    }
    // final_cost(x̄_N) on the raw state (:192; RBD_helper_functions.jl:105-116)
    V lf = V(0);
    if constexpr (TASK) {
      V q[NJ], pw[3];
#pragma unroll
      for (int i = 0; i < NJ; ++i) q[i] = xb[i];
      chain_point_fk<NJ>(P, C, q, pw);
      if constexpr (ROWS) {  // the last step's hand-off left the row in the stage
        ChainTaskK Cb = C;
#pragma unroll
        for (int k = 0; k < 3; ++k) Cb.t[k] = stage[O_G + k];
        lf = chain_task_value(Cb, pw);
      } else {
        lf = chain_task_value(C, pw);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        if constexpr (ROWS) {
          const V e = stage[O_G + i] - xb[i];
          lf = fma(P.qfw[i] * e, e, lf);
        } else {
          const V e = P.tgt[i] - xb[i];
          lf = fma(P.qfw[i] * e, e, lf);
        }
      }
    }
    cost += lf;
    out.trials = trial;
    out.cost = cost;
    if (prev_cost - cost > V(0)) {  // (:77-80); NaN compares false → keep searching
      out.accepted = 1;
      break;
    }
    alpha *= V(ls.shrink);  // (:82)
  }
  if (du2_out) *du2_out = du2;
  return out;
}

// … with the joint-space costs and a goal per trajectory: the rows where the task constants go
template <int NJ, int NU, bool TASK, bool ROWS>
__device__ __forceinline__ ChainFwdOut<double> chain_forward_group32(
    const ChainK<double, NJ>& P, double* __restrict__ stage, int b, int T, const double* __restrict__ x,
    const double* __restrict__ u, const double* __restrict__ xtraj, const double* __restrict__ dg,
    const double* __restrict__ Kg, double prev_cost, double* __restrict__ xnew, double* __restrict__ unew,
    double* du2_out, const LSParams& ls, const ChainGoalRows& G) {
  static_assert(!TASK && ROWS, "the joint-space costs of a handle with a goal per trajectory");
  return chain_forward_group32<NJ, NU, false, true>(P, stage, b, T, x, u, xtraj, dg, Kg, prev_cost, xnew, unew, du2_out,
                                                    ls, ChainTaskK{}, G);
}

constexpr int CH32_WG = 64;  // two trajectories per workgroup (one wave)

// Bytes of a kernel's argument block (each argument at its natural alignment). ChainK is
// passed by value and grows with the joint count — 2,832 bytes at seven joints — beside
// ChainTaskK, ChainIter and LSParams: every forward kernel holds its own block to HIP's
// 4 KB limit, so the largest instantiation is checked where it is compiled.
template <class... A>
constexpr size_t kernarg_bytes() {
  size_t n = 0;
  ((n = (n + alignof(A) - 1) / alignof(A) * alignof(A) + sizeof(A)), ...);
  return n;
}
constexpr size_t HIP_KERNARG_LIMIT = 4096;

// The two forward kernels. TaskK is empty (the joint-space cost) or ChainTaskK (a task mode:
// the TASK instantiation of the group, the task cost's constants one more kernel argument),
// either followed by ChainGoalRows (a goal per trajectory: the ROWS instantiation, the rows'
// pointer one more argument). As a pack it adds nothing to the joint-cost kernels' argument
// list, so every mode keeps the kernel arguments, and with them the code, that each had as a
// kernel written out. A pack in the middle of the list is never deduced: every launch spells
// out <NJ, NU>, <NJ, NU, ChainTaskK>, <NJ, NU, ChainGoalRows> or
// <NJ, NU, ChainTaskK, ChainGoalRows>.
template <class X, class... A>
constexpr int pack_count = (0 + ... + (std::is_same_v<A, X> ? 1 : 0));
// none | ChainTaskK | ChainGoalRows | ChainTaskK, ChainGoalRows
template <class... A>
struct CostPack : std::false_type {};
template <>
struct CostPack<> : std::true_type {};
template <>
struct CostPack<ChainTaskK> : std::true_type {};
template <>
struct CostPack<ChainGoalRows> : std::true_type {};
template <>
struct CostPack<ChainTaskK, ChainGoalRows> : std::true_type {};
template <int NJ, int NU, class... TaskK>
__global__ __launch_bounds__(CH32_WG) void chain_forward32_kernel(
    ChainK<double, NJ> P, TaskK... C, int B, int T, const double* __restrict__ x, const double* __restrict__ u,
    const double* __restrict__ xtraj, const double* __restrict__ d, const double* __restrict__ K,
    const double* __restrict__ prev_cost, double* __restrict__ xnew, double* __restrict__ unew,
    double* __restrict__ new_cost, int32_t* __restrict__ trials, int32_t* __restrict__ status, LSParams ls) {
  static_assert(CostPack<TaskK...>::value, "TaskK: none or ChainTaskK, then none or ChainGoalRows");
  static_assert(kernarg_bytes<ChainK<double, NJ>, TaskK..., int, int, const double*, const double*, const double*,
                              const double*, const double*, const double*, double*, double*, double*, int32_t*,
                              int32_t*, LSParams>() <= HIP_KERNARG_LIMIT,
                "the chain constants by value: the argument block within HIP's limit");
  constexpr int STAGE = ChainStage<NJ, NU>::SIZE;
  __shared__ ChainK<double, NJ> Ps;
  __shared__ double stage[(CH32_WG / CH32_LANES) * STAGE];
  chain_consts_to_lds<CH32_WG>(Ps, P);
  const int b = (blockIdx.x * CH32_WG + threadIdx.x) / CH32_LANES;
  if (b >= B) return;  // the whole lane group
  const int l32 = threadIdx.x & (CH32_LANES - 1);
  const double pc = prev_cost ? prev_cost[b] : (double)INFINITY;
  constexpr bool TASK = pack_count<ChainTaskK, TaskK...> == 1, ROWS = pack_count<ChainGoalRows, TaskK...> == 1;
  const ChainFwdOut<double> r = chain_forward_group32<NJ, NU, TASK, ROWS>(
      Ps, stage + (threadIdx.x / CH32_LANES) * STAGE, b, T, x, u, xtraj, d, K, pc, xnew, unew, nullptr, ls, C...);
  // every lane of the group: the 32 lanes stride the copy of an exhausted search's inputs
  fwd_finish<2 * NJ, NU>(b, T, r.cost, r.trials, r.accepted, x, u, xnew, unew, l32, CH32_LANES, new_cost, trials,
                         status);
}

// fit iteration, forward part. bstatus is the tiles kernel's per-trajectory result of this
// iteration's backward pass (it runs every trajectory): a NaN gain of a running
// trajectory ends it here, as chain_iter_backward4_kernel does
template <int NJ, int NU, class... TaskK>
__global__ __launch_bounds__(CH32_WG) void chain_iter_forward32_kernel(ChainK<double, NJ> P, TaskK... C, int B, int T,
                                                                     ChainIter<double> a,
                                                                     const int32_t* __restrict__ bstatus,
                                                                     LSParams ls) {
  static_assert(CostPack<TaskK...>::value, "TaskK: none or ChainTaskK, then none or ChainGoalRows");
  static_assert(kernarg_bytes<ChainK<double, NJ>, TaskK..., int, int, ChainIter<double>, const int32_t*,
                              LSParams>() <= HIP_KERNARG_LIMIT,
                "the chain constants by value: the argument block within HIP's limit");
  constexpr int STAGE = ChainStage<NJ, NU>::SIZE;
  __shared__ ChainK<double, NJ> Ps;
  __shared__ double stage[(CH32_WG / CH32_LANES) * STAGE];
  chain_consts_to_lds<CH32_WG>(Ps, P);
  const int b = (blockIdx.x * CH32_WG + threadIdx.x) / CH32_LANES;
  if (b >= B || a.status[b] != ILQR_TRAJ_OK) return;  // the whole lane group
  const int l32 = threadIdx.x & (CH32_LANES - 1);
  if (bstatus[b] != ILQR_TRAJ_OK) {  // reference: AssertionError at backward_pass.jl:353
    if (l32 == 0) {
      a.status[b] = ILQR_TRAJ_NAN;
      if (a.res_parity) a.res_parity[b] = a.parity;
    }
    return;
  }
  double du2 = 0.0;
  const double pc = a.prev_cost ? a.prev_cost[b] : (double)INFINITY;
  constexpr bool TASK = pack_count<ChainTaskK, TaskK...> == 1, ROWS = pack_count<ChainGoalRows, TaskK...> == 1;
  const ChainFwdOut<double> r = chain_forward_group32<NJ, NU, TASK, ROWS>(
      Ps, stage + (threadIdx.x / CH32_LANES) * STAGE, b, T, a.x, a.u, a.xtraj, a.d, a.K, pc, a.xnew, a.unew, &du2,
      ls, C...);
  if (l32 != 0) return;
  fwd_iter_finish(a, b, r.cost, r.accepted, r.trials, du2, ls.tol);
}

}  // namespace
}  // namespace ilqr

// ---------------------------------------------------------------------------
// Host side: the chain handle and its C ABI (include/ilqr.h, ilqr_chain_*)
// ---------------------------------------------------------------------------
struct ilqr_chain_handle {
  int device = 0;
  int nj = 0, nu = 0, T = 0, batch = 0;
  int dtype = ILQR_F64;
  int lin = ILQR_LINEARIZE_DUAL;
  ilqr_chain chain{};
  hipStream_t stream = nullptr;
  void* xbuf[2] = {nullptr, nullptr};
  void* ubuf[2] = {nullptr, nullptr};
  void* K = nullptr;
  void* d = nullptr;
  void* J = nullptr;
  // chains on the tiles path (4..7 joints, fp64): the derivative and cost tiles the tiles
  // kernel reads and its per-trajectory status
  double *tA = nullptr, *tB = nullptr, *lx = nullptr, *lu = nullptr, *lxx = nullptr, *luu = nullptr;
  double *lfx = nullptr, *lfxx = nullptr;
  int32_t* bstatus = nullptr;
  ilqr::FitState fit;  // the fit driver's per-trajectory state, words and events (ilqr_fit.h)
  // closed-form dynamics of 2-joint chains (ilqr_chain_set_dynamics): available once
  // sampled and checked against the recursion at creation, used unless RNEA is asked for
  bool trig_ok = false;
  int32_t dyn_mode = ILQR_CHAIN_DYN_AUTO;
  double trig_err = 0.0;  // the check's max relative error
  ilqr::ChainTrig<double> trig{};
  bool use_trig() const { return trig_ok && dyn_mode != ILQR_CHAIN_DYN_RNEA; }
  // cost_functions.jl's factories (ilqr_chain_set_simple_costs): the mode, the chain's
  // joint-space weights as created (restored by ILQR_CHAIN_COST_JOINT) and the
  // task-space final cost's coefficients in device memory
  int32_t cost_mode = ILQR_CHAIN_COST_JOINT;
  ilqr_chain created{};
  ilqr::ChainTask* task_dev = nullptr;
  const ilqr::ChainTask* task() const { return cost_mode == ILQR_CHAIN_COST_JOINT ? nullptr : task_dev; }
  // the same factories on the tiles path (ilqr_chain_set_task_costs): the kinematics are
  // composed on the device, these are the kernel argument
  ilqr::ChainTaskK taskk{};
  bool task_mode() const { return cost_mode != ILQR_CHAIN_COST_JOINT; }
  // a goal per trajectory (ilqr_chain_set_joint_targets, _set_task_targets): the handle's
  // copies of the rows, (batch, n_joints) and (batch, 3), allocated at the first call and
  // kept; `on` while an override is set. Each applies while its cost family is in effect.
  double *joint_rows = nullptr, *task_rows = nullptr;
  bool joint_rows_on = false, task_rows_on = false;
  const double* goal_rows() const {
    return task_mode() ? (task_rows_on ? task_rows : nullptr) : (joint_rows_on ? joint_rows : nullptr);
  }
};

namespace {

thread_local std::string g_chain_error;

ilqr_status chain_hip_fail(hipError_t e, const char* what) {
  g_chain_error = std::string(what) + ": " + hipGetErrorString(e);
  return ILQR_ERR_HIP;
}

#define CH_TRY(expr)                                         \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) return chain_hip_fail(e_, #expr);  \
  } while (0)

template <class V, int NJ>
ilqr::ChainK<V, NJ> chain_consts(const ilqr_chain& c) {
  ilqr::ChainK<V, NJ> P{};
  for (int i = 0; i < NJ; ++i) {
    for (int k = 0; k < 9; ++k) P.R0[i][k] = (V)c.joint_rot[i][k];
    {  // R0·[a]× and R0·a·aᵀ in fp64, then rounded (joint_rot)
      const double* R0 = c.joint_rot[i];
      const double* a = c.axis[i];
      const double ax[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
          double x = 0.0, y = 0.0;
          for (int j = 0; j < 3; ++j) {
            x += R0[3 * r + j] * ax[3 * j + k];
            y += R0[3 * r + j] * a[j] * a[k];
          }
          P.R0x[i][3 * r + k] = (V)x;
          P.R0aa[i][3 * r + k] = (V)y;
        }
    }
    for (int k = 0; k < 3; ++k) {
      P.p[i][k] = (V)c.joint_pos[i][k];
      P.ax[i][k] = (V)c.axis[i][k];
      P.mc[i][k] = (V)(c.mass[i] * c.com[i][k]);
    }
    P.m[i] = (V)c.mass[i];
    // Io = Ic + m(|c|²1 − c cᵀ): rotational inertia about the body origin (fp64 first)
    const double* cm = c.com[i];
    const double cc = cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        P.Io[i][3 * r + k] =
            (V)(c.inertia[i][3 * r + k] + c.mass[i] * ((r == k ? cc : 0.0) - cm[r] * cm[k]));
    P.tgt[i] = (V)c.target[i];
    P.qw[i] = (V)c.q_weight[i];
    P.rw[i] = (V)c.r_weight[i];
    P.qfw[i] = (V)c.qf_weight[i];
  }
  for (int k = 0; k < 3; ++k) P.g[k] = (V)c.gravity[k];
  P.dt = (V)c.dt;
  return P;
}

// ChainTrig<V> from the fp64 coefficients and the chain's cost
template <class V>
ilqr::ChainTrig<V> trig_consts(const ilqr_chain_handle* h) {
  ilqr::ChainTrig<V> Q{};
  const ilqr::ChainTrig<double>& D = h->trig;
  for (int e = 0; e < 3; ++e) {
    for (int k = 0; k < 5; ++k) Q.Mc[e][k] = (V)D.Mc[e][k];
  }
  for (int i = 0; i < 2; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Q.Gc[i][a][b] = (V)D.Gc[i][a][b];
  const ilqr_chain& c = h->chain;
  for (int i = 0; i < 2; ++i) {
    Q.tgt[i] = (V)c.target[i];
    Q.qw[i] = (V)c.q_weight[i];
    Q.rw[i] = (V)c.r_weight[i];
    Q.qfw[i] = (V)c.qf_weight[i];
  }
  Q.dt = (V)c.dt;
  Q.task = h->task();
  return Q;
}

using ilqr::two_pi;

// weight of the sample at angle t in coefficient a of the 3-point discrete Fourier
// transform on φ = (1, cos, sin)
double fourier3(int a, double t) {
  return a == 0 ? 1.0 / 3 : (a == 1 ? 2.0 / 3 * std::cos(t) : 2.0 / 3 * std::sin(t));
}

// Samples M and g with the recursion (fp64, on the device), takes their discrete
// Fourier coefficients (exact for M's degree 2 in q₂ and g's degree 1 in each angle:
// 5 and 3 points), and checks f against the recursion at 256 random states. Leaves
// trig_ok false when the check fails (the recursion is then used).
hipError_t chain_trig_build(ilqr_chain_handle* h) {
  h->trig_ok = false;
  if (h->nj != 2) return hipSuccess;
  const auto P = chain_consts<double, 2>(h->chain);
  constexpr int NCHK = 256;
  double* dev = nullptr;
  hipError_t e = hipMalloc(&dev, sizeof(double) * (ilqr::CH_TRIG_SAMPLES + NCHK));
  if (e != hipSuccess) return e;
  double smp[ilqr::CH_TRIG_SAMPLES], err[NCHK];
  ilqr::chain_trig_sample_kernel<<<1, 64>>>(P, dev);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(smp, dev, sizeof(smp), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    ilqr::ChainTrig<double>& D = h->trig;
    for (int en = 0; en < 3; ++en) {  // a₀ + a₁ cos + b₁ sin + a₂ cos 2 + b₂ sin 2 from 5 samples
      double a0 = 0, a1 = 0, b1 = 0, a2 = 0, b2 = 0;
      for (int k = 0; k < 5; ++k) {
        const double f = smp[3 * k + en], t = two_pi * k / 5.0;
        a0 += f;
        a1 += f * std::cos(t);
        b1 += f * std::sin(t);
        a2 += f * std::cos(2 * t);
        b2 += f * std::sin(2 * t);
      }
      D.Mc[en][0] = a0 / 5;
      D.Mc[en][1] = 2 * a1 / 5;
      D.Mc[en][2] = 2 * b1 / 5;
      D.Mc[en][3] = 2 * a2 / 5;
      D.Mc[en][4] = 2 * b2 / 5;
    }
    for (int i = 0; i < 2; ++i) {  // 2-D transform on the 3×3 grid: φ = (1, cos, sin)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double acc = 0.0;
          for (int ka = 0; ka < 3; ++ka)
            for (int kb = 0; kb < 3; ++kb) {
              const double ta = two_pi * ka / 3.0, tb = two_pi * kb / 3.0;
              const double fa = fourier3(a, ta), fb = fourier3(b, tb);
              acc += smp[15 + 2 * (3 * ka + kb) + i] * fa * fb;
            }
          D.Gc[i][a][b] = acc;
        }
    }
    D.dt = h->chain.dt;
    ilqr::chain_trig_check_kernel<<<NCHK / 64, 64>>>(P, D, NCHK, dev + ilqr::CH_TRIG_SAMPLES);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(err, dev + ilqr::CH_TRIG_SAMPLES, sizeof(err), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  if (e != hipSuccess) return e;
  double m = 0.0;
  for (double v : err) m = std::isnan(v) ? INFINITY : std::max(m, v);
  h->trig_err = m;
  h->trig_ok = m < 1e-9;
  return hipSuccess;
}

// transform_to_root(state, body) * point (RigidBodyDynamics.jl; cost_functions.jl:20): the
// root-frame position of a point given in body `body`'s frame (−1 = the fixed base) at
// joint angles q, composing x_parent = p_i + R0_i·Rot(a_i, q_i)·x_child down the chain (fp64)
void chain_point_position(const ilqr_chain& c, int body, const double pt[3], const double* q,
                          double out[3]) {
  double w[3] = {pt[0], pt[1], pt[2]};
  for (int i = body; i >= 0; --i) {
    const double* a = c.axis[i];
    const double cq = std::cos(q[i]), sq = std::sin(q[i]);
    const double adw = a[0] * w[0] + a[1] * w[1] + a[2] * w[2];
    const double axw[3] = {a[1] * w[2] - a[2] * w[1], a[2] * w[0] - a[0] * w[2], a[0] * w[1] - a[1] * w[0]};
    double r[3];
    for (int k = 0; k < 3; ++k) r[k] = cq * w[k] + sq * axw[k] + (1.0 - cq) * adw * a[k];
    for (int k = 0; k < 3; ++k)
      w[k] = c.joint_pos[i][k] +
             (c.joint_rot[i][3 * k] * r[0] + c.joint_rot[i][3 * k + 1] * r[1] + c.joint_rot[i][3 * k + 2] * r[2]);
  }
  for (int k = 0; k < 3; ++k) out[k] = w[k];
}

// The task cost's coefficients: p sampled on the 3×3 grid of (q₁, q₂) and transformed
// like g's (exact for the bilinear form), then checked against the kinematics at 64
// pseudo-random angles. Returns the check's max deviation relative to the point's reach.
double chain_task_build(const ilqr_chain& c, int body, const double pt[3], const double tgt[3],
                        double weight, bool literal, ilqr::ChainTask& C) {
  double smp[3][3][3];  // [ka][kb][coordinate]
  for (int ka = 0; ka < 3; ++ka)
    for (int kb = 0; kb < 3; ++kb) {
      const double q[2] = {two_pi * ka / 3.0, two_pi * kb / 3.0};
      chain_point_position(c, body, pt, q, smp[ka][kb]);
    }
  double P[3][3][3];
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double acc = 0.0;
        for (int ka = 0; ka < 3; ++ka)
          for (int kb = 0; kb < 3; ++kb) {
            const double ta = two_pi * ka / 3.0, tb = two_pi * kb / 3.0;
            const double fa = fourier3(a, ta), fb = fourier3(b, tb);
            acc += smp[ka][kb][k] * fa * fb;
          }
        P[k][a][b] = acc;
      }
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) C.Pc[k][a][b] = P[literal ? 2 : k][a][b];
  for (int k = 0; k < 3; ++k) C.t[k] = tgt[k];
  C.w = weight;
  double err = 0.0, reach = 1.0;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  for (int n = 0; n < 64; ++n) {
    double q[2];
    for (double& v : q) {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      v = ((double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5) * 4.0 * two_pi;
    }
    double ref[3];
    chain_point_position(c, body, pt, q, ref);
    const double c0 = std::cos(q[0]), s0 = std::sin(q[0]), c1 = std::cos(q[1]), s1 = std::sin(q[1]);
    const double f0[3] = {1.0, c0, s0}, f1[3] = {1.0, c1, s1};
    for (int k = 0; k < 3; ++k) {
      double v = 0.0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) v += P[k][a][b] * f0[a] * f1[b];
      err = std::max(err, std::fabs(v - ref[k]));
      reach = std::max(reach, std::fabs(ref[k]));
    }
  }
  return err / reach;
}

// h->lin as a compile-time constant: fn(std::integral_constant<int, LIN>{}), for the kernels
// that carry both modes (ILQR_LINEARIZE_ANALYTIC is a kernel of its own, tiles path only:
// ChainTilesOps::linearize branches to it before coming here)
template <class Fn>
hipError_t with_lin(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->lin == ILQR_LINEARIZE_DUAL) return fn(std::integral_constant<int, ILQR_LINEARIZE_DUAL>{});
  return fn(std::integral_constant<int, ILQR_LINEARIZE_CENTRAL_FD>{});
}

size_t vsize(const ilqr_chain_handle* h) { return h->dtype == ILQR_F32 ? 4 : 8; }

// Typed operations of one (V, NJ, NU) instantiation. The iteration's parts (linearize,
// backward, forward, iteration) exist for two joints only: the recursion is
// chain_backward4's, four 4 × 4 trajectories per wave. Another joint count answers
// `dynamics` alone (four to seven joints iterate through ChainTilesOps).
template <class V, int NJ, int NU>
struct ChainOps {
  static constexpr int NX = 2 * NJ;
  using Value = V;
  using Iter = ilqr::ChainIter<V>;

  static hipError_t linearize(ilqr_chain_handle* h, const V* x, const V* u, const int32_t* st) {
    static_assert(NJ == 2, "ChainOps iterates 2-joint chains only");
    const auto P = chain_consts<V, NJ>(h->chain);
    const size_t lanes = (size_t)h->batch * h->T * (NX + NU);
    const dim3 grid((unsigned)((lanes + 255) / 256));
    if (h->use_trig()) {
      const auto Q = trig_consts<V>(h);
      return with_lin(h, [&](auto lin) {
        ilqr::chain_linearize_kernel<V, NJ, NU, decltype(lin)::value, ilqr::ChainTrig<V>>
            <<<grid, 256, 0, h->stream>>>(Q, h->batch, h->T, x, u, st, (V*)h->J);
        return hipGetLastError();
      });
    }
    return with_lin(h, [&](auto lin) {
      ilqr::chain_linearize_kernel<V, NJ, NU, decltype(lin)::value>
          <<<grid, 256, 0, h->stream>>>(P, h->batch, h->T, x, u, st, (V*)h->J);
      return hipGetLastError();
    });
  }
  static hipError_t unpack(ilqr_chain_handle* h, V* A, V* Bm) {
    const size_t n = (size_t)h->batch * h->T;
    ilqr::chain_unpack_kernel<V, NJ, NU><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
        h->batch, h->T, (const V*)h->J, A, Bm);
    return hipGetLastError();
  }
  // ilqr_chain_linearize: the records, then the caller's A and B
  static hipError_t linearize_to(ilqr_chain_handle* h, const V* x, const V* u, V* A, V* Bm) {
    hipError_t e = linearize(h, x, u, nullptr);
    return e != hipSuccess ? e : unpack(h, A, Bm);
  }
  static hipError_t backward(ilqr_chain_handle* h, const V* x, const V* u, V* d, V* K,
                             int32_t* st, double mu) {
    static_assert(NJ == 2, "ChainOps iterates 2-joint chains only");
    hipError_t e = linearize(h, x, u, nullptr);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    // four trajectories per wave on the f64 MFMA
    ilqr::chain_backward4_kernel<V, NU><<<(h->batch + 15) / 16, 256, 0, h->stream>>>(
        P, h->batch, h->T, x, (const V*)h->J, d, K, st, (V)mu, h->task());
    return hipGetLastError();
  }
  static hipError_t forward(ilqr_chain_handle* h, const V* x, const V* u, const V* xt, const V* d,
                            const V* K, const V* pc, V* xn, V* un, V* nc, int32_t* tr,
                            int32_t* st, const ilqr::LSParams& ls) {
    static_assert(NJ == 2, "ChainOps iterates 2-joint chains only");
    if (h->use_trig()) {
      if (!ilqr::fg_fits<V>(h->T)) return hipErrorInvalidValue;
      const auto Q = trig_consts<V>(h);
      const int B = h->batch;
      return ilqr::fg_with_lanes(B, false, [&](auto g) {
        using G = decltype(g);
        ilqr::chain_forward_trig_kernel<V, NU, G::L, G::W><<<G::blocks(B), G::threads, 0, h->stream>>>(
            Q, B, h->T, x, u, xt, d, K, pc, xn, un, nc, tr, st, ls);
        return hipGetLastError();
      });
    }
    const auto P = chain_consts<V, NJ>(h->chain);
    ilqr::chain_forward_kernel<V, NJ, NU><<<(h->batch * ilqr::CH_FW_LANES + ilqr::CH_WG - 1) / ilqr::CH_WG, ilqr::CH_WG,
                                            0, h->stream>>>(P, h->batch, h->T, x, u, xt, d, K, pc,
                                                            xn, un, nc, tr, st, ls);
    return hipGetLastError();
  }
  static hipError_t iteration(ilqr_chain_handle* h, const Iter& a, const ilqr::LSParams& ls) {
    static_assert(NJ == 2, "ChainOps iterates 2-joint chains only");
    hipError_t e = linearize(h, a.x, a.u, a.status);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    ilqr::chain_iter_backward4_kernel<V, NU>
        <<<(h->batch + 15) / 16, 256, 0, h->stream>>>(P, h->batch, h->T, a, (const V*)h->J, (V)ls.mu, h->task());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (h->use_trig()) {
      if (!ilqr::fg_fits<V>(h->T)) return hipErrorInvalidValue;
      const auto Q = trig_consts<V>(h);
      const int B = h->batch;
      return ilqr::fg_with_lanes(B, a.iter >= 2, [&](auto g) {  // wide: a fit past its first iteration
        using G = decltype(g);
        ilqr::chain_iter_forward_trig_kernel<V, NU, G::L, G::W>
            <<<G::blocks(B), G::threads, 0, h->stream>>>(Q, B, h->T, a, ls);
        return hipGetLastError();
      });
    }
    const int gf = (h->batch * ilqr::CH_FW_LANES + ilqr::CH_WG - 1) / ilqr::CH_WG;
    ilqr::chain_iter_forward_kernel<V, NJ, NU><<<gf, ilqr::CH_WG, 0, h->stream>>>(P, h->batch, h->T,
                                                                                 a, ls);
    return hipGetLastError();
  }
  static hipError_t dynamics(ilqr_chain_handle* h, const V* x, const V* u, V* xo, int n) {
    if constexpr (NJ == 2) {
      if (h->use_trig()) {
        ilqr::chain_dynamics_kernel<V, NJ, NU, ilqr::ChainTrig<V>>
            <<<(n + 255) / 256, 256, 0, h->stream>>>(trig_consts<V>(h), n, x, u, xo);
        return hipGetLastError();
      }
    }
    const auto P = chain_consts<V, NJ>(h->chain);
    ilqr::chain_dynamics_kernel<V, NJ, NU><<<(n + 255) / 256, 256, 0, h->stream>>>(P, n, x, u, xo);
    return hipGetLastError();
  }
};

// Chains of NJ = 4..7 joints, every joint driven (nu = NJ, fp64): ChainOps' interface on the
// tiles path — the linearisation and the costs written as tiles,
// launch_tiles_backward(2·NJ, NJ), the 32-lane forward group.
template <int NJ_>
struct ChainTilesOps {
  static constexpr int NJ = NJ_, NU = NJ_, NX = 2 * NJ_;
  static_assert(NJ > 3 && NJ + 1 <= 8, "the 32-lane forward group: one role per Newton-Euler pass");
  using Value = double;
  using V = double;
  using Iter = ilqr::ChainIter<double>;

  static ilqr::ChainCostK<NJ> cost_consts(const ilqr_chain& c) {
    ilqr::ChainCostK<NJ> C{};
    for (int i = 0; i < NJ; ++i) {
      C.tgt[i] = c.target[i];
      C.qw[i] = c.q_weight[i];
      C.rw[i] = c.r_weight[i];
      C.qfw[i] = c.qf_weight[i];
    }
    return C;
  }
  // lxx, luu, lfxx of the handle's cost in effect: at ilqr_chain_create and at every change
  // of the cost mode (in a task mode h->chain carries q = 0, r = 1, qf = 0: lxx = 0,
  // luu = 2I, and lfxx is rewritten by every backward)
  static hipError_t hessians(ilqr_chain_handle* h) {
    const size_t n = (size_t)h->batch * (h->T + 1) * NX * NX;
    ilqr::chain_cost_hessians_kernel<NJ, NU><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
        cost_consts(h->chain), h->batch, h->T, h->lxx, h->luu, h->lfxx);
    return hipGetLastError();
  }
  // A and B of trajectories with status OK (st null: all)
  static hipError_t linearize(ilqr_chain_handle* h, const V* x, const V* u, const int32_t* st, V* A, V* Bm) {
    const auto P = chain_consts<V, NJ>(h->chain);
    if (h->lin == ILQR_LINEARIZE_ANALYTIC) {  // 64 / (NX + NU) points per wave, four waves
      const size_t per_wg = 4 * (64 / (NX + NU)), wgs = ((size_t)h->batch * h->T + per_wg - 1) / per_wg;
      ilqr::chain_linearize_analytic_kernel<NJ><<<dim3((unsigned)wgs), 256, 0, h->stream>>>(
          P, h->batch, h->T, x, u, st, A, Bm);
      return hipGetLastError();
    }
    const size_t lanes = (size_t)h->batch * h->T * (NX + NU);
    const dim3 grid((unsigned)((lanes + 255) / 256));
    return with_lin(h, [&](auto lin) {
      ilqr::chain_linearize_tiles_kernel<NJ, NU, decltype(lin)::value>
          <<<grid, 256, 0, h->stream>>>(P, h->batch, h->T, x, u, st, A, Bm);
      return hipGetLastError();
    });
  }
  // ilqr_chain_linearize: the name its generic lambda calls on ChainOps and ChainTilesOps alike
  static hipError_t linearize_to(ilqr_chain_handle* h, const V* x, const V* u, V* A, V* Bm) {
    return linearize(h, x, u, nullptr, A, Bm);
  }
  // the step's tiles, likewise
  static hipError_t tiles(ilqr_chain_handle* h, const V* x, const V* u, const int32_t* st) {
    hipError_t e = linearize(h, x, u, st, h->tA, h->tB);
    if (e != hipSuccess) return e;
    const size_t n = (size_t)h->batch * (h->T + 1) * (NX + NU);
    if (const double* rows = h->goal_rows(); rows && !h->task_mode())  // θ* per trajectory
      ilqr::chain_cost_tiles_kernel<NJ, NU, ilqr::ChainGoalRows><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
          cost_consts(h->chain), ilqr::ChainGoalRows{rows}, h->batch, h->T, x, u, st, h->lx, h->lu, h->lfx);
    else
      ilqr::chain_cost_tiles_kernel<NJ, NU><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
          cost_consts(h->chain), h->batch, h->T, x, u, st, h->lx, h->lu, h->lfx);
    if ((e = hipGetLastError()) != hipSuccess || !h->task_mode()) return e;
    // a task mode: lx = 0 and lu = 2u came from the weights above; the terminal tiles from x_N
    return quadratize(h, x + (size_t)h->T * NX, (size_t)(h->T + 1) * NX, h->batch, st, nullptr, h->lfx, h->lfxx);
  }
  // final_cost_quadratization of the cost in effect at n states x[s·stride .. +NX); with a
  // goal per trajectory of that cost, state s against row s (the callers hold n to batch)
  static hipError_t quadratize(ilqr_chain_handle* h, const V* x, size_t stride, int n, const int32_t* st, V* cost,
                               V* grad, V* hess) {
    if (const double* rows = h->goal_rows())
      ilqr::chain_task_quad_kernel<NJ, ilqr::ChainGoalRows><<<(n + 63) / 64, 64, 0, h->stream>>>(
          chain_consts<V, NJ>(h->chain), h->taskk, ilqr::ChainGoalRows{rows}, h->task_mode() ? 0 : 1, n, x, stride,
          st, cost, grad, hess);
    else
      ilqr::chain_task_quad_kernel<NJ><<<(n + 63) / 64, 64, 0, h->stream>>>(
          chain_consts<V, NJ>(h->chain), h->taskk, h->task_mode() ? 0 : 1, n, x, stride, st, cost, grad, hess);
    return hipGetLastError();
  }
  static ilqr::TileParams tile_params(const ilqr_chain_handle* h) {
    return ilqr::TileParams{h->tA, h->tB, h->lx, h->lu, h->lxx, nullptr, h->luu, h->lfx, h->lfxx};
  }
  static hipError_t backward(ilqr_chain_handle* h, const V* x, const V* u, V* d, V* K, int32_t* st,
                             double mu) {
    hipError_t e = tiles(h, x, u, nullptr);
    if (e != hipSuccess) return e;
    return ilqr::launch_tiles_backward(NX, NU, tile_params(h), h->batch, h->T, d, K, st ? st : h->bstatus, mu,
                                       h->stream);
  }
  static hipError_t forward(ilqr_chain_handle* h, const V* x, const V* u, const V* xt, const V* d,
                            const V* K, const V* pc, V* xn, V* un, V* nc, int32_t* tr, int32_t* st,
                            const ilqr::LSParams& ls) {
    const auto P = chain_consts<V, NJ>(h->chain);
    const int grid = (h->batch * ilqr::CH32_LANES + ilqr::CH32_WG - 1) / ilqr::CH32_WG;
    const ilqr::ChainGoalRows rows{h->goal_rows()};  // a goal per trajectory of the cost in effect
    if (rows.rows && h->task_mode())
      ilqr::chain_forward32_kernel<NJ, NU, ilqr::ChainTaskK, ilqr::ChainGoalRows>
          <<<grid, ilqr::CH32_WG, 0, h->stream>>>(P, h->taskk, rows, h->batch, h->T, x, u, xt, d, K, pc, xn, un, nc,
                                                  tr, st, ls);
    else if (rows.rows)
      ilqr::chain_forward32_kernel<NJ, NU, ilqr::ChainGoalRows><<<grid, ilqr::CH32_WG, 0, h->stream>>>(
          P, rows, h->batch, h->T, x, u, xt, d, K, pc, xn, un, nc, tr, st, ls);
    else if (h->task_mode())
      ilqr::chain_forward32_kernel<NJ, NU, ilqr::ChainTaskK><<<grid, ilqr::CH32_WG, 0, h->stream>>>(
          P, h->taskk, h->batch, h->T, x, u, xt, d, K, pc, xn, un, nc, tr, st, ls);
    else
      ilqr::chain_forward32_kernel<NJ, NU><<<grid, ilqr::CH32_WG, 0, h->stream>>>(P, h->batch, h->T, x, u, xt, d, K,
                                                                               pc, xn, un, nc, tr, st, ls);
    return hipGetLastError();
  }
  static hipError_t iteration(ilqr_chain_handle* h, const Iter& a, const ilqr::LSParams& ls) {
    hipError_t e = tiles(h, a.x, a.u, a.status);
    if (e != hipSuccess) return e;
    // every trajectory runs the recursion (a stopped one on stale tiles, into the handle's
    // own gains); the forward kernel folds bstatus into the running ones' status
    e = ilqr::launch_tiles_backward(NX, NU, tile_params(h), h->batch, h->T, a.d, a.K, h->bstatus, ls.mu,
                                    h->stream);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    const int grid = (h->batch * ilqr::CH32_LANES + ilqr::CH32_WG - 1) / ilqr::CH32_WG;
    const ilqr::ChainGoalRows rows{h->goal_rows()};
    if (rows.rows && h->task_mode())
      ilqr::chain_iter_forward32_kernel<NJ, NU, ilqr::ChainTaskK, ilqr::ChainGoalRows>
          <<<grid, ilqr::CH32_WG, 0, h->stream>>>(P, h->taskk, rows, h->batch, h->T, a, h->bstatus, ls);
    else if (rows.rows)
      ilqr::chain_iter_forward32_kernel<NJ, NU, ilqr::ChainGoalRows><<<grid, ilqr::CH32_WG, 0, h->stream>>>(
          P, rows, h->batch, h->T, a, h->bstatus, ls);
    else if (h->task_mode())
      ilqr::chain_iter_forward32_kernel<NJ, NU, ilqr::ChainTaskK><<<grid, ilqr::CH32_WG, 0, h->stream>>>(
          P, h->taskk, h->batch, h->T, a, h->bstatus, ls);
    else
      ilqr::chain_iter_forward32_kernel<NJ, NU><<<grid, ilqr::CH32_WG, 0, h->stream>>>(P, h->batch, h->T, a,
                                                                                    h->bstatus, ls);
    return hipGetLastError();
  }
};

// (n_joints, nu) shapes with compiled kernels in every dtype: the iLQR iteration for the
// 2-DoF arm (nu = 2 every joint driven, nu = 1 joint 1 only); dynamics also for the shapes
// of the tiles path: 4..7 joints, every joint driven (three joints have no 32-lane group,
// eight joints' nine Newton-Euler passes do not fit its eight roles).
bool iter_supported(int nj, int nu) { return nj == 2 && (nu == 1 || nu == 2); }
bool tiles_shape(int nj, int nu) { return nj >= 4 && nj <= 7 && nu == nj; }
bool dyn_supported(int nj, int nu) { return iter_supported(nj, nu) || tiles_shape(nj, nu); }
// ... and per dtype: the tiles path iterates in fp64 only (its recursion is the f64 MFMA
// tiles kernel)
bool iter_supported_dtype(int nj, int nu, int32_t dtype) {
  if (dtype != ILQR_F32 && dtype != ILQR_F64) return false;
  return iter_supported(nj, nu) || (tiles_shape(nj, nu) && dtype == ILQR_F64);
}
bool handle_iterates(const ilqr_chain_handle* h) { return iter_supported_dtype(h->nj, h->nu, h->dtype); }
// the handle iterates on the tiles path: its workspace is the tiles, its cost modes
// ilqr_chain_set_task_costs'
bool on_tiles(const ilqr_chain_handle* h) { return tiles_shape(h->nj, h->nu) && handle_iterates(h); }

// fn(the handle's typed operations). DYN: the call is ilqr_chain_dynamics, which every
// dyn_supported shape answers from ChainOps in either dtype; otherwise the shapes and
// dtypes that iterate.
template <class V, bool DYN, int NJ, class Fn>
hipError_t dispatch_tiles(Fn&& fn) {
  if constexpr (DYN) return fn(ChainOps<V, NJ, NJ>{});
  else if constexpr (std::is_same_v<V, double>) return fn(ChainTilesOps<NJ>{});
  else return hipErrorInvalidValue;
}
template <class V, bool DYN = false, class Fn>
hipError_t dispatch(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->nj == 2 && h->nu == 2) return fn(ChainOps<V, 2, 2>{});
  if (h->nj == 2 && h->nu == 1) return fn(ChainOps<V, 2, 1>{});
  if (tiles_shape(h->nj, h->nu)) switch (h->nj) {
      case 4: return dispatch_tiles<V, DYN, 4>(fn);
      case 5: return dispatch_tiles<V, DYN, 5>(fn);
      case 6: return dispatch_tiles<V, DYN, 6>(fn);
      case 7: return dispatch_tiles<V, DYN, 7>(fn);
    }
  return hipErrorInvalidValue;
}
// fn(ChainTilesOps<nj>{}) of a handle on the tiles path
template <class Fn>
hipError_t with_tiles_ops(const ilqr_chain_handle* h, Fn&& fn) {
  if (on_tiles(h)) switch (h->nj) {
      case 4: return fn(ChainTilesOps<4>{});
      case 5: return fn(ChainTilesOps<5>{});
      case 6: return fn(ChainTilesOps<6>{});
      case 7: return fn(ChainTilesOps<7>{});
    }
  return hipErrorInvalidValue;
}
template <bool DYN = false, class Fn>
hipError_t dispatch_any(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->dtype == ILQR_F32) return dispatch<float, DYN>(h, fn);
  return dispatch<double, DYN>(h, fn);
}

template <class V>
ilqr::ChainIter<V> iter_args(const ilqr_chain_handle* h, const void* x, const void* u,
                             const void* xt, void* xn, void* un, const void* pc, void* nc,
                             void* du2, int32_t* tr, int32_t* st) {
  ilqr::ChainIter<V> a{};
  a.x = (const V*)x;
  a.u = (const V*)u;
  a.xtraj = (const V*)xt;
  a.xnew = (V*)xn;
  a.unew = (V*)un;
  a.K = (V*)h->K;
  a.d = (V*)h->d;
  a.prev_cost = (const V*)pc;
  a.new_cost = (V*)nc;
  a.du2 = (V*)du2;
  a.trials = tr;
  a.status = st;
  return a;
}

template <class V>
ilqr_status chain_fit_t(ilqr_chain_handle* h, const ilqr_options* o, const void* x_init,
                        const void* u_init, const void* x_traj, void* x_out, void* u_out,
                        void* cost, int32_t* iters, int32_t* status, const ilqr_history* hist) {
  // The shared fit driver (ilqr_fit.h, DESIGN.md §4 fit driver) around this family's iteration
  hipStream_t s = h->stream;
  ilqr::FitState& f = h->fit;
  const ilqr::LSParams ls = ilqr::ls_params(o);
  ilqr::FitCall c;
  c.B = h->batch, c.T = h->T, c.nx = 2 * h->nj, c.nu = h->nu;
  c.f32 = sizeof(V) == 4;
  c.max_iter = o ? o->max_iter : 100;
  c.x_init = x_init, c.u_init = u_init, c.x_out = x_out, c.u_out = u_out;
  for (int i = 0; i < 2; ++i) c.xbuf[i] = h->xbuf[i], c.ubuf[i] = h->ubuf[i];
  CH_TRY(ilqr::fit_begin(f, c, x_traj, ls.tol, /*init=*/true, s));
  for (int it = 1; it <= c.max_iter; ++it) {  // forward_pass.jl:161
    const ilqr::FitBuffers b = ilqr::fit_buffers(c, it);
    auto a = iter_args<V>(h, b.x, b.u, x_traj, b.xnew, b.unew, f.prev_cost, f.prev_cost, f.du2, f.trials, f.status);
    a.res_parity = f.res_parity;
    a.iters = f.iters;
    a.parity = b.parity;
    a.iter = it;
    CH_TRY(dispatch<V>(h, [&](auto ops) { return decltype(ops)::iteration(h, a, ls); }));
    if (hist)  // the per-iteration record (ilqr_history)
      CH_TRY(ilqr::launch_record_history(h->batch, it, f.status, f.iters, f.trials, f.prev_cost, f.du2, c.f32,
                                         ls.alpha0, ls.shrink, hist->cost, hist->trials, hist->alpha, hist->du2,
                                         s));
    bool stopped;
    CH_TRY(ilqr::fit_poll(f, c, it, s, &stopped));
    if (stopped) break;
  }
  ilqr_status st = ILQR_OK;
  CH_TRY(ilqr::fit_end(f, c, cost, iters, status, s, &st));
  return st;
}

// The argument check of the two cost entries (ilqr_chain_set_simple_costs, _set_task_costs):
// the mode, and what a task mode reads
ilqr_status check_cost_args(const ilqr_chain_handle* h, int32_t mode, int32_t body, const double* point,
                            const double* final_target, double weight) {
  if (mode != ILQR_CHAIN_COST_JOINT && mode != ILQR_CHAIN_COST_SIMPLE &&
      mode != ILQR_CHAIN_COST_SIMPLE_EUCLIDEAN)
    return ILQR_ERR_BAD_ARG;
  if (mode == ILQR_CHAIN_COST_JOINT) return ILQR_OK;  // the joint-space costs: nothing else is read
  if (!point || !final_target || !std::isfinite(weight)) return ILQR_ERR_BAD_ARG;
  if (body < -1 || body >= h->nj) return ILQR_ERR_BAD_ARG;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(point[k]) || !std::isfinite(final_target[k])) return ILQR_ERR_BAD_ARG;
  return ILQR_OK;
}

// The weights the kernels read in cost mode `mode`: the handle's own as created in the joint
// mode, ℓ = Σu² in a task mode (simple_immediate_cost, cost_functions.jl:45-51: q = 0, r = 1,
// qf = 0). The caller has made sure no launch in flight still reads the old ones.
void apply_cost_mode(ilqr_chain_handle* h, int32_t mode) {
  h->chain = h->created;
  if (mode != ILQR_CHAIN_COST_JOINT)
    for (int i = 0; i < ILQR_CHAIN_MAX_JOINTS; ++i) {
      h->chain.q_weight[i] = 0.0;
      h->chain.r_weight[i] = 1.0;
      h->chain.qf_weight[i] = 0.0;
    }
  h->cost_mode = mode;
}

// lxx, luu, lfxx of a handle on the tiles path, for its cost in effect
hipError_t tiles_hessians(ilqr_chain_handle* h) {
  return with_tiles_ops(h, [&](auto ops) { return decltype(ops)::hessians(h); });
}

// The cost mode of a handle on the tiles path: the weights the per-step tiles and the forward
// read and the Hessian tiles that go with them, enqueued on the handle's stream as at creation
// (launches take the weights by value, in stream order). h->taskk is set by the caller.
ilqr_status chain_tiles_set_cost_mode(ilqr_chain_handle* h, int32_t mode) {
  CH_TRY(hipSetDevice(h->device));
  apply_cost_mode(h, mode);
  CH_TRY(tiles_hessians(h));
  return ILQR_OK;
}

// ilqr_chain_set_joint_targets / _set_task_targets: (batch, width) device doubles into the
// handle's own buffer (allocated at the first call, kept until ilqr_chain_destroy) by a
// device-to-device copy on the handle's stream, after the launches already enqueued there
// and waited for, so that the caller's array is free when the call returns. NULL clears the
// override and keeps the buffer.
ilqr_status chain_set_goal_rows(ilqr_chain_handle* h, const double* targets, size_t width, double** rows, bool* on,
                                const char* who) {
  if (!on_tiles(h)) {
    g_chain_error = std::string(who) + ": needs a handle that iterates on the tiles path (4 to 7 joints, fp64)";
    return ILQR_ERR_UNSUPPORTED;
  }
  if (!targets) {
    *on = false;
    return ILQR_OK;
  }
  const size_t bytes = sizeof(double) * (size_t)h->batch * width;
  CH_TRY(hipSetDevice(h->device));
  if (!*rows) CH_TRY(hipMalloc(rows, bytes));
  CH_TRY(hipMemcpyAsync(*rows, targets, bytes, hipMemcpyDeviceToDevice, h->stream));
  CH_TRY(hipStreamSynchronize(h->stream));
  *on = true;
  return ILQR_OK;
}

}  // namespace

extern "C" {

int ilqr_chain_supported(int n_joints, int nu) { return iter_supported(n_joints, nu) ? 1 : 0; }

int ilqr_chain_supported_dtype(int n_joints, int nu, int32_t dtype) {
  return iter_supported_dtype(n_joints, nu, dtype) ? 1 : 0;
}

const char* ilqr_chain_last_error(void) { return g_chain_error.c_str(); }

ilqr_status ilqr_chain_create(ilqr_chain_handle** out, int device, const ilqr_chain* chain, int T,
                              int batch, int32_t dtype, int32_t linearization) {
  if (!out || !chain) return ILQR_ERR_BAD_ARG;
  *out = nullptr;
  if (T <= 0 || batch <= 0 || chain->n_joints <= 0 || chain->nu <= 0) return ILQR_ERR_BAD_DIMS;
  if (chain->n_joints > ILQR_CHAIN_MAX_JOINTS || !(chain->nu == chain->n_joints || chain->nu == 1))
    return ILQR_ERR_BAD_DIMS;
  if (dtype != ILQR_F32 && dtype != ILQR_F64) return ILQR_ERR_BAD_ARG;
  if (linearization != ILQR_LINEARIZE_DUAL && linearization != ILQR_LINEARIZE_CENTRAL_FD &&
      linearization != ILQR_LINEARIZE_ANALYTIC)
    return ILQR_ERR_BAD_ARG;
  if (!(chain->dt > 0.0)) return ILQR_ERR_BAD_ARG;
  if (!dyn_supported(chain->n_joints, chain->nu)) return ILQR_ERR_UNSUPPORTED;
  if (linearization == ILQR_LINEARIZE_ANALYTIC &&
      !(tiles_shape(chain->n_joints, chain->nu) && dtype == ILQR_F64)) {
    g_chain_error = "ilqr_chain_create: ILQR_LINEARIZE_ANALYTIC is the tiles path's (4 to 7 joints, "
                    "every joint driven, ILQR_F64)";
    return ILQR_ERR_UNSUPPORTED;
  }
  CH_TRY(hipSetDevice(device));
  auto* h = new ilqr_chain_handle;
  h->device = device;
  h->nj = chain->n_joints;
  h->nu = chain->nu;
  h->T = T;
  h->batch = batch;
  h->dtype = dtype;
  h->lin = linearization;
  h->chain = *chain;
  h->created = *chain;
  const size_t w = vsize(h), B = (size_t)batch, nx = 2 * (size_t)h->nj, nu = (size_t)h->nu;
  hipError_t e = hipSuccess;
  const bool tiles = on_tiles(h);
  if (handle_iterates(h)) {  // dynamics-only shapes need no workspace
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipMalloc(&h->xbuf[i], w * B * (T + 1) * nx);
      if (e == hipSuccess) e = hipMalloc(&h->ubuf[i], w * B * T * nu);
    }
    if (e == hipSuccess) e = hipMalloc(&h->K, w * B * T * nu * nx);
    if (e == hipSuccess) e = hipMalloc(&h->d, w * B * T * nu);
    if (e == hipSuccess && !tiles) e = hipMalloc(&h->J, w * B * T * (nx * (nx + nu) + nx + nu));
    if (tiles) {  // the tiles in place of the records
      auto tile = [&](double** p, size_t n) {
        if (e == hipSuccess) e = hipMalloc(p, sizeof(double) * n);
      };
      tile(&h->tA, B * T * nx * nx);
      tile(&h->tB, B * T * nx * nu);
      tile(&h->lx, B * T * nx);
      tile(&h->lu, B * T * nu);
      tile(&h->lxx, B * T * nx * nx);
      tile(&h->luu, B * T * nu * nu);
      tile(&h->lfx, B * nx);
      tile(&h->lfxx, B * nx * nx);
      if (e == hipSuccess) e = hipMalloc(&h->bstatus, sizeof(int32_t) * B);
      // stopped trajectories run the recursion on whatever their tiles hold: keep it defined
      if (e == hipSuccess) e = hipMemset(h->tA, 0, sizeof(double) * B * T * nx * nx);
      if (e == hipSuccess) e = hipMemset(h->tB, 0, sizeof(double) * B * T * nx * nu);
      if (e == hipSuccess) e = hipMemset(h->lx, 0, sizeof(double) * B * T * nx);
      if (e == hipSuccess) e = hipMemset(h->lu, 0, sizeof(double) * B * T * nu);
      if (e == hipSuccess) e = hipMemset(h->lfx, 0, sizeof(double) * B * nx);
    }
    if (e == hipSuccess) e = ilqr::fit_state_create(&h->fit, B, w);
  }
  if (e != hipSuccess) {
    ilqr_chain_destroy(h);
    return chain_hip_fail(e, "ilqr_chain_create: hipMalloc");
  }
  if (iter_supported(h->nj, h->nu) && (e = chain_trig_build(h)) != hipSuccess) {
    ilqr_chain_destroy(h);
    return chain_hip_fail(e, "ilqr_chain_create: closed-form dynamics");
  }
  if (tiles) {
    e = tiles_hessians(h);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      ilqr_chain_destroy(h);
      return chain_hip_fail(e, "ilqr_chain_create: cost tiles");
    }
  }
  *out = h;
  return ILQR_OK;
}

ilqr_status ilqr_chain_set_dynamics(ilqr_chain_handle* h, int32_t mode) {
  if (!h) return ILQR_ERR_BAD_ARG;
  if (mode != ILQR_CHAIN_DYN_AUTO && mode != ILQR_CHAIN_DYN_RNEA && mode != ILQR_CHAIN_DYN_CLOSED_FORM)
    return ILQR_ERR_BAD_ARG;
  if (mode == ILQR_CHAIN_DYN_CLOSED_FORM && !h->trig_ok) return ILQR_ERR_UNSUPPORTED;
  // the task-space final cost is evaluated by the closed-form forward only
  // (2-joint chains; the tiles path composes the kinematics beside the recursion)
  if (mode == ILQR_CHAIN_DYN_RNEA && h->cost_mode != ILQR_CHAIN_COST_JOINT && iter_supported(h->nj, h->nu))
    return ILQR_ERR_UNSUPPORTED;
  h->dyn_mode = mode;
  return ILQR_OK;
}

ilqr_status ilqr_chain_set_simple_costs(ilqr_chain_handle* h, int32_t mode, int32_t body,
                                        const double* point, const double* final_target,
                                        double weight) {
  if (!h) return ILQR_ERR_BAD_ARG;
  const ilqr_status st = check_cost_args(h, mode, body, point, final_target, weight);
  if (st != ILQR_OK) return st;
  if (mode == ILQR_CHAIN_COST_JOINT) {  // the joint-space costs the handle was created with
    if (h->cost_mode != ILQR_CHAIN_COST_JOINT) {
      if (on_tiles(h)) return chain_tiles_set_cost_mode(h, ILQR_CHAIN_COST_JOINT);  // its tiles too
      CH_TRY(hipStreamSynchronize(h->stream));  // launches in flight still read the old cost
      apply_cost_mode(h, ILQR_CHAIN_COST_JOINT);
    }
    return ILQR_OK;
  }
  if (!iter_supported(h->nj, h->nu) || !h->use_trig()) {
    g_chain_error = "ilqr_chain_set_simple_costs: needs a 2-joint chain on the closed-form dynamics";
    return ILQR_ERR_UNSUPPORTED;
  }
  ilqr::ChainTask C{};
  const double err =
      chain_task_build(h->created, body, point, final_target, weight, mode == ILQR_CHAIN_COST_SIMPLE, C);
  if (!(err < 1e-12)) {
    g_chain_error = "ilqr_chain_set_simple_costs: the point's coordinates are not bilinear in "
                    "(cos, sin) of the joint angles (kinematics check failed)";
    return ILQR_ERR_UNSUPPORTED;
  }
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(hipStreamSynchronize(h->stream));
  if (!h->task_dev) CH_TRY(hipMalloc(&h->task_dev, sizeof(ilqr::ChainTask)));
  CH_TRY(hipMemcpy(h->task_dev, &C, sizeof(C), hipMemcpyHostToDevice));
  apply_cost_mode(h, mode);
  return ILQR_OK;
}

ilqr_status ilqr_chain_set_task_costs(ilqr_chain_handle* h, int32_t mode, int32_t body, const double* point,
                                      const double* final_target, double weight) {
  if (!h) return ILQR_ERR_BAD_ARG;
  // 2-joint chains: the sampled closed form, with its returns
  if (iter_supported(h->nj, h->nu)) return ilqr_chain_set_simple_costs(h, mode, body, point, final_target, weight);
  const ilqr_status st = check_cost_args(h, mode, body, point, final_target, weight);
  if (st != ILQR_OK) return st;
  if (mode == ILQR_CHAIN_COST_JOINT)
    return h->cost_mode == ILQR_CHAIN_COST_JOINT ? ILQR_OK : chain_tiles_set_cost_mode(h, ILQR_CHAIN_COST_JOINT);
  if (!on_tiles(h)) {
    g_chain_error = "ilqr_chain_set_task_costs: needs a handle that iterates on the tiles path (4 to 7 joints, fp64)";
    return ILQR_ERR_UNSUPPORTED;
  }
  for (int k = 0; k < 3; ++k) {
    h->taskk.pt[k] = point[k];
    h->taskk.t[k] = final_target[k];
  }
  h->taskk.w = weight;
  h->taskk.body = body;
  h->taskk.literal = mode == ILQR_CHAIN_COST_SIMPLE ? 1 : 0;
  return chain_tiles_set_cost_mode(h, mode);
}

ilqr_status ilqr_chain_final_cost_quadratize(ilqr_chain_handle* h, const void* x, int n, void* cost, void* grad,
                                             void* hess) {
  if (!h || !x) return ILQR_ERR_BAD_ARG;
  if (n <= 0) return ILQR_ERR_BAD_DIMS;
  if (!on_tiles(h)) return ILQR_ERR_UNSUPPORTED;
  if (h->goal_rows() && n != h->batch) return ILQR_ERR_BAD_DIMS;  // state s against row s
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(with_tiles_ops(h, [&](auto ops) {
    using O = decltype(ops);
    return O::quadratize(h, (const double*)x, O::NX, n, nullptr, (double*)cost, (double*)grad, (double*)hess);
  }));
  return ILQR_OK;
}

int32_t ilqr_chain_get_cost_mode(const ilqr_chain_handle* h) { return h ? h->cost_mode : -1; }

ilqr_status ilqr_chain_set_joint_targets(ilqr_chain_handle* h, const double* targets) {
  if (!h) return ILQR_ERR_BAD_ARG;
  return chain_set_goal_rows(h, targets, (size_t)h->nj, &h->joint_rows, &h->joint_rows_on,
                             "ilqr_chain_set_joint_targets");
}

ilqr_status ilqr_chain_set_task_targets(ilqr_chain_handle* h, const double* targets) {
  if (!h) return ILQR_ERR_BAD_ARG;
  return chain_set_goal_rows(h, targets, 3, &h->task_rows, &h->task_rows_on, "ilqr_chain_set_task_targets");
}

int32_t ilqr_chain_get_target_mode(const ilqr_chain_handle* h) {
  return h ? (h->joint_rows_on ? 1 : 0) | (h->task_rows_on ? 2 : 0) : -1;
}

int32_t ilqr_chain_get_dynamics(const ilqr_chain_handle* h) {
  if (!h) return -1;
  return h->use_trig() ? ILQR_CHAIN_DYN_CLOSED_FORM : ILQR_CHAIN_DYN_RNEA;
}

double ilqr_chain_closed_form_error(const ilqr_chain_handle* h) { return h ? h->trig_err : -1.0; }

ilqr_status ilqr_chain_destroy(ilqr_chain_handle* h) {
  if (!h) return ILQR_OK;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < 2; ++i) {
    (void)hipFree(h->xbuf[i]);
    (void)hipFree(h->ubuf[i]);
  }
  for (void* p : {h->K, h->d, h->J}) (void)hipFree(p);
  for (double* p : {h->tA, h->tB, h->lx, h->lu, h->lxx, h->luu, h->lfx, h->lfxx}) (void)hipFree(p);
  (void)hipFree(h->bstatus);
  ilqr::fit_state_destroy(&h->fit);
  (void)hipFree(h->task_dev);
  (void)hipFree(h->joint_rows);
  (void)hipFree(h->task_rows);
  delete h;
  return ILQR_OK;
}

ilqr_status ilqr_chain_set_stream(ilqr_chain_handle* h, void* s) {
  if (!h) return ILQR_ERR_BAD_ARG;
  h->stream = (hipStream_t)s;
  return ILQR_OK;
}

ilqr_status ilqr_chain_dynamics(ilqr_chain_handle* h, const void* x, const void* u, void* x_next,
                                int n) {
  if (!h || !x || !u || !x_next) return ILQR_ERR_BAD_ARG;
  if (n <= 0) return ILQR_ERR_BAD_DIMS;
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(dispatch_any<true>(h, [&](auto ops) {
    using O = decltype(ops);
    using V = typename O::Value;
    return O::dynamics(h, (const V*)x, (const V*)u, (V*)x_next, n);
  }));
  return ILQR_OK;
}

ilqr_status ilqr_chain_linearize(ilqr_chain_handle* h, const void* x, const void* u, void* A,
                                 void* B) {
  if (!h || !x || !u || !A || !B) return ILQR_ERR_BAD_ARG;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(dispatch_any(h, [&](auto ops) {
    using O = decltype(ops);
    using V = typename O::Value;
    return O::linearize_to(h, (const V*)x, (const V*)u, (V*)A, (V*)B);
  }));
  return ILQR_OK;
}

ilqr_status ilqr_chain_backward(ilqr_chain_handle* h, const ilqr_options* o, const void* x,
                                const void* u, void* d, void* K, int32_t* status) {
  if (!h || !x || !u || !d || !K) return ILQR_ERR_BAD_ARG;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  ilqr_status st = ilqr::check_options(o);
  if (st != ILQR_OK) return st;
  CH_TRY(hipSetDevice(h->device));
  const double mu = ilqr::ls_params(o).mu;
  CH_TRY(dispatch_any(h, [&](auto ops) {
    using O = decltype(ops);
    using V = typename O::Value;
    return O::backward(h, (const V*)x, (const V*)u, (V*)d, (V*)K, status, mu);
  }));
  if (status) CH_TRY(ilqr::fold_status(status, h->batch, h->stream, nullptr, &st));
  return st;
}

ilqr_status ilqr_chain_forward(ilqr_chain_handle* h, const ilqr_options* o, const void* x,
                               const void* u, const void* x_traj, const void* d, const void* K,
                               const void* prev_cost, void* x_new, void* u_new, void* new_cost,
                               int32_t* trials, int32_t* status) {
  if (!h || !x || !u || !d || !K || !prev_cost || !x_new || !u_new || !new_cost)
    return ILQR_ERR_BAD_ARG;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  ilqr_status st = ilqr::check_options(o);
  if (st != ILQR_OK) return st;
  CH_TRY(hipSetDevice(h->device));
  const ilqr::LSParams ls = ilqr::ls_params(o);
  CH_TRY(dispatch_any(h, [&](auto ops) {
    using O = decltype(ops);
    using V = typename O::Value;
    return O::forward(h, (const V*)x, (const V*)u, (const V*)x_traj, (const V*)d, (const V*)K,
                      (const V*)prev_cost, (V*)x_new, (V*)u_new, (V*)new_cost, trials, status, ls);
  }));
  if (status) CH_TRY(ilqr::fold_status(status, h->batch, h->stream, nullptr, &st));
  return st;
}

ilqr_status ilqr_chain_iterate(ilqr_chain_handle* h, const ilqr_options* o, const void* x,
                               const void* u, const void* x_traj, void* x_new, void* u_new,
                               const void* prev_cost, void* new_cost, void* du2, int32_t* trials,
                               int32_t* status) {
  if (!h || !x || !u || !x_new || !u_new || !new_cost || !status) return ILQR_ERR_BAD_ARG;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  ilqr_status st = ilqr::check_options(o);
  if (st != ILQR_OK) return st;
  CH_TRY(hipSetDevice(h->device));
  const ilqr::LSParams ls = ilqr::ls_params(o);
  CH_TRY(dispatch_any(h, [&](auto ops) {
    using O = decltype(ops);
    using V = typename O::Value;
    const auto a = iter_args<V>(h, x, u, x_traj, x_new, u_new, prev_cost, new_cost, du2, trials,
                                status);
    return O::iteration(h, a, ls);
  }));
  return ILQR_OK;
}

ilqr_status ilqr_chain_fit(ilqr_chain_handle* h, const ilqr_options* o, const void* x_init,
                           const void* u_init, const void* x_traj, void* x_out, void* u_out,
                           void* cost, int32_t* iters, int32_t* status) {
  return ilqr_chain_fit_ex(h, o, x_init, u_init, x_traj, x_out, u_out, cost, iters, status, nullptr);
}

ilqr_status ilqr_chain_fit_ex(ilqr_chain_handle* h, const ilqr_options* o, const void* x_init,
                              const void* u_init, const void* x_traj, void* x_out, void* u_out,
                              void* cost, int32_t* iters, int32_t* status, const ilqr_history* hist) {
  if (!h || !x_init || !u_init || !x_out || !u_out) return ILQR_ERR_BAD_ARG;
  if (hist && !hist->cost && !hist->trials && !hist->alpha && !hist->du2) hist = nullptr;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  ilqr_status st = ilqr::check_options(o);
  if (st != ILQR_OK) return st;
  CH_TRY(hipSetDevice(h->device));
  if (h->dtype == ILQR_F32)
    return chain_fit_t<float>(h, o, x_init, u_init, x_traj, x_out, u_out, cost, iters, status, hist);
  return chain_fit_t<double>(h, o, x_init, u_init, x_traj, x_out, u_out, cost, iters, status, hist);
}

ilqr_status ilqr_chain_sync(ilqr_chain_handle* h) {
  if (!h) return ILQR_ERR_BAD_ARG;
  CH_TRY(hipStreamSynchronize(h->stream));
  return ILQR_OK;
}

}  // extern "C"
