// MI355X (gfx950) kernels of 2-joint chains + the C ABI of the RBD problem family
// (ILQR_PROBLEM_CHAIN): a fixed-base serial chain of revolute joints described by a URDF —
// the reference's RigidBodyDynamics.jl example (test/RBD_2_link_example/
// RBD_helper_functions.jl:48-116 on test/urdf/2Dof_arm.urdf; BASELINE.json
// config 5) with a fixed base. The family is three pieces: the rigid-body
// model both paths share (ilqr_chain_model.h), this file, and the tiles path of 4 to 7
// joints (ilqr_chain_tiles.hip, one object per joint count, reached through
// ilqr_chain_host.h's ChainTilesTable).
//
// What replaces what:
//  * dynamicsf (:48-79): RK4 of v̇ = M(q) \ (τ − dynamics_bias(q, v)), q̇ = v. The
//    device functor is Featherstone's recursive Newton-Euler (the published
//    algorithm behind RBD.jl's dynamics_bias) for the bias, and M's columns from the
//    same recursion with unit accelerations; everything templated on the scalar
//    (float / double / DualT<N, ·>) — ilqr_chain_model.h. Here: its closed form for two
//    joints (ChainTrig), the default of the iteration kernels.
//  * linearize_dynamics (src/backward_pass.jl:25-40, ForwardDiff): forward-mode dual
//    numbers (ILQR_LINEARIZE_DUAL, exact like the reference) or central finite
//    differences (ILQR_LINEARIZE_CENTRAL_FD, what BASELINE config 5 names), one lane
//    per (trajectory, step, direction).
//  * immediate_cost / final_cost (:85-116) on the joint rows: Σ qwᵢ(θ*ᵢ−θᵢ)² + Σ rwₖuₖ²
//    and Σ qfwᵢ(θ*ᵢ−θᵢ)²; their derivatives are the exact constants.
//  * backward_pass / forward_pass / fit: the Riccati recursion, four trajectories per
//    wave on the 4-block f64 MFMA, and the RK4 rollout + α-halving line search (the shared
//    forward group on the closed form, a 16-lane group per trajectory on the
//    component-parallel Newton-Euler otherwise), in the handle's dtype (fp32 or fp64).
//  * cost_functions.jl's simple_final_cost / simple_immediate_cost (src/cost_functions.jl:
//    5-54) in place of the joint-space costs: the point's coordinates as a polynomial
//    sampled at the call (ChainTask, ilqr_chain_set_simple_costs, closed-form dynamics
//    only). ilqr_chain_set_simple_costs keeps refusing more than two joints, and an fp32
//    handle of more than two joints answers dynamics only.
// Layout as the other families (include/ilqr.h): x (B, T+1, nx), u/d (B, T, nu),
// K (B, T, nu, nx), trajectory slowest, nx = 2·n_joints.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "ilqr_chain_host.h"
#include "ilqr_fwd_group.h"

namespace ilqr {
namespace {

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

template <class V_, int NU_>
__device__ __forceinline__ void ChainTrigModel<V_, NU_>::rk4_robust(const V (&x)[4], const V (&u)[NU],
                                                                   V (&o)[4]) const {
  chain_rk4<2, NU>(P, x, u, o);
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

}  // namespace
}  // namespace ilqr

// ---------------------------------------------------------------------------
// Host side: the chain handle and its C ABI (include/ilqr.h, ilqr_chain_*)
// ---------------------------------------------------------------------------
namespace {

thread_local std::string g_chain_error;

#define CH_TRY(expr) ILQR_HIP_TRY(g_chain_error, expr)

// a buffer the handle acquires at its first use and keeps (through its owner, which a failed
// request must not poison for the next call: an optional request, reported here)
template <class T>
hipError_t chain_lazy_dev(ilqr_chain_handle* h, T** p, size_t count) {
  return *p || h->own.try_dev(p, count) ? hipSuccess : hipErrorOutOfMemory;
}

// ChainTrig<V> from the fp64 coefficients and the chain's cost
template <class V>
ilqr::ChainTrig<V> trig_consts(const ilqr_chain_handle* h) {
  ilqr::ChainTrig<V> Q{};
  const ilqr::ChainTrig<double>& D = h->two.trig;
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
  Q.task = h->two.task(h->task_mode());
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
  h->two.trig_ok = false;
  if (h->nj != 2) return hipSuccess;
  const auto P = chain_consts<double, 2>(h->chain);
  constexpr int NCHK = 256;
  double* dev = nullptr;
  ilqr::HipOwned tmp;  // the sample buffer, released on every exit
  tmp.set_device(h->device);
  tmp.dev(&dev, ilqr::CH_TRIG_SAMPLES + NCHK);
  hipError_t e = tmp.error();
  if (e != hipSuccess) return e;
  double smp[ilqr::CH_TRIG_SAMPLES], err[NCHK];
  ilqr::chain_trig_sample_kernel<<<1, 64>>>(P, dev);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(smp, dev, sizeof(smp), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    ilqr::ChainTrig<double>& D = h->two.trig;
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
  if (e != hipSuccess) return e;
  double m = 0.0;
  for (double v : err) m = std::isnan(v) ? INFINITY : std::max(m, v);
  h->two.trig_err = m;
  h->two.trig_ok = m < 1e-9;
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

size_t vsize(const ilqr_chain_handle* h) { return h->dtype == ILQR_F32 ? 4 : 8; }

// Typed operations of one (V, 2, NU) instantiation: two joints only, the recursion is
// chain_backward4's, four 4 × 4 trajectories per wave (four to seven joints: the
// ChainTilesTable of their joint count).
template <class V, int NJ, int NU>
struct ChainOps {
  static_assert(NJ == 2, "ChainOps is the 2-joint chains'");
  static constexpr int NX = 2 * NJ;
  using Value = V;
  using Iter = ilqr::ChainIter<V>;

  static hipError_t linearize(ilqr_chain_handle* h, const V* x, const V* u, const int32_t* st) {
    const auto P = chain_consts<V, NJ>(h->chain);
    const size_t lanes = (size_t)h->batch * h->T * (NX + NU);
    const dim3 grid((unsigned)((lanes + 255) / 256));
    if (h->two.use_trig()) {
      const auto Q = trig_consts<V>(h);
      return with_lin(h, [&](auto lin) {
        ilqr::chain_linearize_kernel<V, NJ, NU, decltype(lin)::value, ilqr::ChainTrig<V>>
            <<<grid, 256, 0, h->stream>>>(Q, h->batch, h->T, x, u, st, (V*)h->two.J);
        return hipGetLastError();
      });
    }
    return with_lin(h, [&](auto lin) {
      ilqr::chain_linearize_kernel<V, NJ, NU, decltype(lin)::value>
          <<<grid, 256, 0, h->stream>>>(P, h->batch, h->T, x, u, st, (V*)h->two.J);
      return hipGetLastError();
    });
  }
  static hipError_t unpack(ilqr_chain_handle* h, V* A, V* Bm) {
    const size_t n = (size_t)h->batch * h->T;
    ilqr::chain_unpack_kernel<V, NJ, NU><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
        h->batch, h->T, (const V*)h->two.J, A, Bm);
    return hipGetLastError();
  }
  // ilqr_chain_linearize: the records, then the caller's A and B
  static hipError_t linearize_to(ilqr_chain_handle* h, const V* x, const V* u, V* A, V* Bm) {
    hipError_t e = linearize(h, x, u, nullptr);
    return e != hipSuccess ? e : unpack(h, A, Bm);
  }
  static hipError_t backward(ilqr_chain_handle* h, const V* x, const V* u, V* d, V* K,
                             int32_t* st, double mu) {
    hipError_t e = linearize(h, x, u, nullptr);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    // four trajectories per wave on the f64 MFMA
    ilqr::chain_backward4_kernel<V, NU><<<(h->batch + 15) / 16, 256, 0, h->stream>>>(
        P, h->batch, h->T, x, (const V*)h->two.J, d, K, st, (V)mu, h->two.task(h->task_mode()));
    return hipGetLastError();
  }
  static hipError_t forward(ilqr_chain_handle* h, const V* x, const V* u, const V* xt, const V* d,
                            const V* K, const V* pc, V* xn, V* un, V* nc, int32_t* tr,
                            int32_t* st, const ilqr::LSParams& ls) {
    if (h->two.use_trig()) {
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
    hipError_t e = linearize(h, a.x, a.u, a.status);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    ilqr::chain_iter_backward4_kernel<V, NU>
        <<<(h->batch + 15) / 16, 256, 0, h->stream>>>(P, h->batch, h->T, a, (const V*)h->two.J, (V)ls.mu, h->two.task(h->task_mode()));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (h->two.use_trig()) {
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
    if (h->two.use_trig()) {
      ilqr::chain_dynamics_kernel<V, NJ, NU, ilqr::ChainTrig<V>>
          <<<(n + 255) / 256, 256, 0, h->stream>>>(trig_consts<V>(h), n, x, u, xo);
      return hipGetLastError();
    }
    const auto P = chain_consts<V, NJ>(h->chain);
    ilqr::chain_dynamics_kernel<V, NJ, NU><<<(n + 255) / 256, 256, 0, h->stream>>>(P, n, x, u, xo);
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

// the table of a handle that iterates on the tiles path, or null
const ilqr::ChainTilesTable* tiles_table(const ilqr_chain_handle* h) {
  return on_tiles(h) ? ilqr::chain_tiles_table(h->nj) : nullptr;
}

// fn(ops) with the handle's operations in V: ChainOps of a 2-joint handle, or the tiles
// path's table (fp64), whose entries are called like ChainOps' members
template <class V, class Fn>
hipError_t dispatch(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->nj == 2 && h->nu == 2) return fn(ChainOps<V, 2, 2>{});
  if (h->nj == 2 && h->nu == 1) return fn(ChainOps<V, 2, 1>{});
  if constexpr (std::is_same_v<V, double>)
    if (const ilqr::ChainTilesTable* t = tiles_table(h)) return fn(*t);
  return hipErrorInvalidValue;
}
template <class Fn>
hipError_t dispatch_any(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->dtype == ILQR_F32) return dispatch<float>(h, fn);
  return dispatch<double>(h, fn);
}

// a fit iteration's arguments in ChainIter's field order; the fit driver's fields stay null / 0
template <class V>
ilqr::ChainIter<V> iter_args(const ilqr_chain_handle* h, const void* x, const void* u,
                             const void* xt, void* xn, void* un, const void* pc, void* nc,
                             void* du2, int32_t* tr, int32_t* st) {
  return ilqr::ChainIter<V>{(const V*)x, (const V*)u, (const V*)xt, (V*)xn, (V*)un, (V*)h->K,
                            (V*)h->d,    (const V*)pc, (V*)nc,       (V*)du2, tr,     st};
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
    CH_TRY(dispatch<V>(h, [&](const auto& ops) { return ops.iteration(h, a, ls); }));
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

// The cost mode of a handle on the tiles path: the weights the per-step tiles and the forward
// read and the Hessian tiles that go with them, enqueued on the handle's stream as at creation
// (launches take the weights by value, in stream order). h->tiles.taskk is set by the caller.
ilqr_status chain_tiles_set_cost_mode(ilqr_chain_handle* h, int32_t mode) {
  CH_TRY(hipSetDevice(h->device));
  apply_cost_mode(h, mode);
  CH_TRY(tiles_table(h)->hessians(h));
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
  CH_TRY(chain_lazy_dev(h, rows, (size_t)h->batch * width));
  CH_TRY(hipMemcpyAsync(*rows, targets, bytes, hipMemcpyDeviceToDevice, h->stream));
  CH_TRY(hipStreamSynchronize(h->stream));
  *on = true;
  return ILQR_OK;
}

}  // namespace

const ilqr::ChainTilesTable* ilqr::chain_tiles_table(int nj) {
  static const ChainTilesTable* const tables[] = {&chain_tiles_table_4, &chain_tiles_table_5, &chain_tiles_table_6,
                                                  &chain_tiles_table_7};
  return nj >= 4 && nj <= 7 ? tables[nj - 4] : nullptr;
}

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
  const bool tiles = on_tiles(h);
  ilqr::HipOwned& own = h->own;
  own.set_device(device);
  hipError_t e = hipSuccess;
  if (handle_iterates(h)) {  // dynamics-only shapes need no workspace
    for (int i = 0; i < 2; ++i) {
      own.dev(&h->xbuf[i], w * B * (T + 1) * nx);
      own.dev(&h->ubuf[i], w * B * T * nu);
    }
    own.dev(&h->K, w * B * T * nu * nx);
    own.dev(&h->d, w * B * T * nu);
    if (!tiles) own.dev(&h->two.J, w * B * T * (nx * (nx + nu) + nx + nu));
    if (tiles) {  // the tiles in place of the records
      ilqr_chain_handle::Tiles& t = h->tiles;
      // zeroed: stopped trajectories run the recursion on whatever their tiles hold
      own.dev_zero(&t.tA, B * T * nx * nx);
      own.dev_zero(&t.tB, B * T * nx * nu);
      own.dev_zero(&t.lx, B * T * nx);
      own.dev_zero(&t.lu, B * T * nu);
      own.dev_zero(&t.lxx, B * T * nx * nx);
      own.dev_zero(&t.luu, B * T * nu * nu);
      own.dev_zero(&t.lfx, B * nx);
      own.dev_zero(&t.lfxx, B * nx * nx);
      own.dev(&t.bstatus, B);
    }
    e = ilqr::fit_state_create(&h->fit, own, B, w);
  }
  if (e != hipSuccess) {
    delete h;
    return ilqr::hip_fail(g_chain_error, e, "ilqr_chain_create: hipMalloc");
  }
  if (iter_supported(h->nj, h->nu) && (e = chain_trig_build(h)) != hipSuccess) {
    delete h;
    return ilqr::hip_fail(g_chain_error, e, "ilqr_chain_create: closed-form dynamics");
  }
  if (tiles) {
    e = tiles_table(h)->hessians(h);  // lxx, luu, lfxx of the cost in effect
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      delete h;
      return ilqr::hip_fail(g_chain_error, e, "ilqr_chain_create: cost tiles");
    }
  }
  *out = h;
  return ILQR_OK;
}

ilqr_status ilqr_chain_set_dynamics(ilqr_chain_handle* h, int32_t mode) {
  if (!h) return ILQR_ERR_BAD_ARG;
  if (mode != ILQR_CHAIN_DYN_AUTO && mode != ILQR_CHAIN_DYN_RNEA && mode != ILQR_CHAIN_DYN_CLOSED_FORM)
    return ILQR_ERR_BAD_ARG;
  if (mode == ILQR_CHAIN_DYN_CLOSED_FORM && !h->two.trig_ok) return ILQR_ERR_UNSUPPORTED;
  // the task-space final cost is evaluated by the closed-form forward only
  // (2-joint chains; the tiles path composes the kinematics beside the recursion)
  if (mode == ILQR_CHAIN_DYN_RNEA && h->cost_mode != ILQR_CHAIN_COST_JOINT && iter_supported(h->nj, h->nu))
    return ILQR_ERR_UNSUPPORTED;
  h->two.dyn_mode = mode;
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
  if (!iter_supported(h->nj, h->nu) || !h->two.use_trig()) {
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
  CH_TRY(chain_lazy_dev(h, &h->two.task_dev, 1));
  CH_TRY(hipMemcpy(h->two.task_dev, &C, sizeof(C), hipMemcpyHostToDevice));
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
    h->tiles.taskk.pt[k] = point[k];
    h->tiles.taskk.t[k] = final_target[k];
  }
  h->tiles.taskk.w = weight;
  h->tiles.taskk.body = body;
  h->tiles.taskk.literal = mode == ILQR_CHAIN_COST_SIMPLE ? 1 : 0;
  return chain_tiles_set_cost_mode(h, mode);
}

ilqr_status ilqr_chain_final_cost_quadratize(ilqr_chain_handle* h, const void* x, int n, void* cost, void* grad,
                                             void* hess) {
  if (!h || !x) return ILQR_ERR_BAD_ARG;
  if (n <= 0) return ILQR_ERR_BAD_DIMS;
  if (!on_tiles(h)) return ILQR_ERR_UNSUPPORTED;
  if (h->tiles.goal_rows(h->task_mode()) && n != h->batch) return ILQR_ERR_BAD_DIMS;  // state s against row s
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(tiles_table(h)->quadratize(h, (const double*)x, 2 * (size_t)h->nj, n, nullptr, (double*)cost, (double*)grad,
                                    (double*)hess));
  return ILQR_OK;
}

int32_t ilqr_chain_get_cost_mode(const ilqr_chain_handle* h) { return h ? h->cost_mode : -1; }

ilqr_status ilqr_chain_set_joint_targets(ilqr_chain_handle* h, const double* targets) {
  if (!h) return ILQR_ERR_BAD_ARG;
  return chain_set_goal_rows(h, targets, (size_t)h->nj, &h->tiles.joint_rows, &h->tiles.joint_rows_on,
                             "ilqr_chain_set_joint_targets");
}

ilqr_status ilqr_chain_set_task_targets(ilqr_chain_handle* h, const double* targets) {
  if (!h) return ILQR_ERR_BAD_ARG;
  return chain_set_goal_rows(h, targets, 3, &h->tiles.task_rows, &h->tiles.task_rows_on, "ilqr_chain_set_task_targets");
}

// The path as chain_set_goal_rows takes its rows — the handle's own buffers, acquired at the
// first call and kept, filled by device-to-device copies on the handle's stream and waited
// for — plus the compact copy of the rows T that the goal-row kernels read. lxx is written by
// every backward while the path applies, so clearing it in a task mode restores the mode's
// constant Hessian tiles (a change of the cost mode does that itself).
ilqr_status ilqr_chain_set_task_path(ilqr_chain_handle* h, const double* path, double path_weight) {
  if (!h) return ILQR_ERR_BAD_ARG;
  if (!on_tiles(h)) {
    g_chain_error = "ilqr_chain_set_task_path: needs a handle that iterates on the tiles path (4 to 7 joints, fp64)";
    return ILQR_ERR_UNSUPPORTED;
  }
  ilqr_chain_handle::Tiles& t = h->tiles;
  if (!path) {
    if (!t.path_on) return ILQR_OK;
    t.path_on = false;
    if (!h->task_mode()) return ILQR_OK;
    CH_TRY(hipSetDevice(h->device));
    CH_TRY(tiles_table(h)->hessians(h));
    return ILQR_OK;
  }
  if (!std::isfinite(path_weight)) return ILQR_ERR_BAD_ARG;
  const size_t B = (size_t)h->batch, row = 3 * sizeof(double), traj = row * ((size_t)h->T + 1);
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(chain_lazy_dev(h, &t.path, B * ((size_t)h->T + 1) * 3));
  CH_TRY(chain_lazy_dev(h, &t.path_goal, B * 3));
  CH_TRY(hipMemcpyAsync(t.path, path, B * traj, hipMemcpyDeviceToDevice, h->stream));
  CH_TRY(hipMemcpy2DAsync(t.path_goal, row, path + 3 * (size_t)h->T, traj, row, B, hipMemcpyDeviceToDevice, h->stream));
  CH_TRY(hipStreamSynchronize(h->stream));
  t.path_weight = path_weight;
  t.path_on = true;
  return ILQR_OK;
}

// Joint-velocity weights: host values the launches take by value, in stream order. lxx and
// lfxx carry them on the velocity diagonal, so setting, replacing and clearing enqueue the
// Hessian tiles of the cost in effect as a change of the cost mode does (with a tool path in
// effect every backward rewrites lxx anyway).
ilqr_status ilqr_chain_set_velocity_weights(ilqr_chain_handle* h, const double* v_weight, const double* vf_weight) {
  if (!h) return ILQR_ERR_BAD_ARG;
  if (!on_tiles(h)) {
    g_chain_error =
        "ilqr_chain_set_velocity_weights: needs a handle that iterates on the tiles path (4 to 7 joints, fp64)";
    return ILQR_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < h->nj; ++i)
    if ((v_weight && !std::isfinite(v_weight[i])) || (vf_weight && !std::isfinite(vf_weight[i])))
      return ILQR_ERR_BAD_ARG;
  ilqr_chain_handle::Tiles& t = h->tiles;
  const bool on = v_weight || vf_weight;
  if (!on && !t.vel_on) return ILQR_OK;
  for (int i = 0; i < ILQR_CHAIN_MAX_JOINTS; ++i) {
    t.v_weight[i] = v_weight && i < h->nj ? v_weight[i] : 0.0;
    t.vf_weight[i] = vf_weight && i < h->nj ? vf_weight[i] : 0.0;
  }
  t.vel_on = on;
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(tiles_table(h)->hessians(h));
  return ILQR_OK;
}

int32_t ilqr_chain_get_velocity_weights(const ilqr_chain_handle* h, double* v_weight, double* vf_weight) {
  if (!h) return -1;
  for (int i = 0; i < h->nj; ++i) {
    if (v_weight) v_weight[i] = h->tiles.vel_on ? h->tiles.v_weight[i] : 0.0;
    if (vf_weight) vf_weight[i] = h->tiles.vel_on ? h->tiles.vf_weight[i] : 0.0;
  }
  return h->tiles.vel_on ? 1 : 0;
}

int32_t ilqr_chain_get_target_mode(const ilqr_chain_handle* h) {
  return h ? (h->tiles.joint_rows_on ? 1 : 0) | (h->tiles.task_rows_on ? 2 : 0) | (h->tiles.path_on ? 4 : 0) : -1;
}

int32_t ilqr_chain_get_dynamics(const ilqr_chain_handle* h) {
  if (!h) return -1;
  return h->two.use_trig() ? ILQR_CHAIN_DYN_CLOSED_FORM : ILQR_CHAIN_DYN_RNEA;
}

double ilqr_chain_closed_form_error(const ilqr_chain_handle* h) { return h ? h->two.trig_err : -1.0; }

ilqr_status ilqr_chain_destroy(ilqr_chain_handle* h) {
  delete h;  // its owner releases
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
  if (h->dtype == ILQR_F32 && tiles_shape(h->nj, h->nu))  // a dynamics-only handle
    CH_TRY(ilqr::chain_tiles_table(h->nj)->dynamics_f32(h, (const float*)x, (const float*)u, (float*)x_next, n));
  else
    CH_TRY(dispatch_any(h, [&](const auto& ops) {
      using V = typename std::decay_t<decltype(ops)>::Value;
      return ops.dynamics(h, (const V*)x, (const V*)u, (V*)x_next, n);
    }));
  return ILQR_OK;
}

ilqr_status ilqr_chain_linearize(ilqr_chain_handle* h, const void* x, const void* u, void* A,
                                 void* B) {
  if (!h || !x || !u || !A || !B) return ILQR_ERR_BAD_ARG;
  if (!handle_iterates(h)) return ILQR_ERR_UNSUPPORTED;
  CH_TRY(hipSetDevice(h->device));
  CH_TRY(dispatch_any(h, [&](const auto& ops) {
    using V = typename std::decay_t<decltype(ops)>::Value;
    return ops.linearize_to(h, (const V*)x, (const V*)u, (V*)A, (V*)B);
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
  CH_TRY(dispatch_any(h, [&](const auto& ops) {
    using V = typename std::decay_t<decltype(ops)>::Value;
    return ops.backward(h, (const V*)x, (const V*)u, (V*)d, (V*)K, status, mu);
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
  CH_TRY(dispatch_any(h, [&](const auto& ops) {
    using V = typename std::decay_t<decltype(ops)>::Value;
    return ops.forward(h, (const V*)x, (const V*)u, (const V*)x_traj, (const V*)d, (const V*)K,
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
  CH_TRY(dispatch_any(h, [&](const auto& ops) {
    using V = typename std::decay_t<decltype(ops)>::Value;
    return ops.iteration(h, iter_args<V>(h, x, u, x_traj, x_new, u_new, prev_cost, new_cost, du2, trials, status), ls);
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
