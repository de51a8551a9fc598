// The rigid-body model of the RBD chain family (ILQR_PROBLEM_CHAIN), device side, shared by
// the chain objects: ilqr_chain.hip (2-joint chains and the C ABI) and ilqr_chain_tiles.hip
// (4 to 7 joints, one object per joint count). The scalar helpers and dual numbers, the
// chain constants (ChainK), the recursive Newton-Euler pass in its scalar and its
// component-parallel form, chain_xdot / chain_rk4, the dynamics kernel, the argument structs
// the handle stores (ilqr_chain_host.h) and the few types both forward families share.
// Everything sits in ilqr's unnamed namespace: each object compiles its own internal copies.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "../../include/ilqr.h"
#include "ilqr_device.h"
#include "ilqr_math.h"

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

// ---------------------------------------------------------------------------
// Kernel arguments the handle keeps (ilqr_chain_host.h): ChainTask and ChainTrig of the
// 2-joint closed form (ilqr_chain.hip), ChainTaskK of the tiles path (ilqr_chain_tiles.hip)
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

template <class V>
struct ChainTrig {
  V Mc[3][5];     // M₀₀, M₀₁, M₁₁: a₀ + a₁ cos q₂ + b₁ sin q₂ + a₂ cos 2q₂ + b₂ sin 2q₂
  V Gc[2][3][3];  // g_i = Σ_ab Gc[i][a][b] φ_a(q₁) φ_b(q₂), φ = (1, cos, sin)
  V dt;
  V tgt[2], qw[2], rw[2], qfw[2];  // joint-space cost (as ChainK)
  const ChainTask* task;           // the task-space final cost in place of qfw's, or null
};
// [q̇; v̇] of the closed form, defined beside it (ilqr_chain.hip): chain_rk4 names it
template <int NU, class S, class V>
__device__ __forceinline__ void chain_xdot_trig(const ChainTrig<V>& P, const S (&x)[4], const S (&u)[NU],
                                                S (&xd)[4]);

// the task-space costs' constants on the tiles path: the point's kinematics are composed on
// the device (chain_point_fk)
struct ChainTaskK {
  double pt[3];     // the point in body `body`'s frame
  double t[3];      // final_target
  double w;         // weight
  int32_t body;     // −1 (the fixed base) .. NJ − 1
  int32_t literal;  // the reference's reading: p_z against every target component
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

// ---------------------------------------------------------------------------
// What the forward families share: a line search's result, the fit iteration's arguments,
// the constants' copy to LDS and the size of a kernel's argument block
// ---------------------------------------------------------------------------
template <class V>
struct ChainFwdOut {
  V cost;
  int trials;
  int accepted;
};

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

// The chain constants go to LDS in the forward kernels: as a kernel argument they overflow
// the SGPR file (~210 SGPRs spilled to VGPR lanes at every use). WG threads copy and meet.
template <int WG, class PK>
__device__ __forceinline__ void chain_consts_to_lds(PK& Ps, const PK& P) {
  static_assert(sizeof(PK) % 4 == 0, "dword copy");
  for (int i = threadIdx.x; i < (int)(sizeof(PK) / 4); i += WG)
    reinterpret_cast<uint32_t*>(&Ps)[i] = reinterpret_cast<const uint32_t*>(&P)[i];
  __syncthreads();
}

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

}  // namespace
}  // namespace ilqr
