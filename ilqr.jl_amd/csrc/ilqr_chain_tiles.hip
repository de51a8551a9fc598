// MI355X (gfx950) kernels of the RBD chain family (ilqr_chain.hip, ILQR_PROBLEM_CHAIN) on the
// tiles path: four to seven joints, every joint driven (the 6-DoF arm, a 7-DoF manipulator),
// iterating in fp64. Compiled once per joint count (-DILQR_CHAIN_NJ=4, 5, 6, 7: every
// instantiation here is one joint count's, and the dual-number linearisation alone is most of
// the family's compile time), each object defining its ChainTilesTable (ilqr_chain_host.h),
// through which the C ABI in ilqr_chain.hip reaches it.
//  * linearize_dynamics: dual numbers or central differences, one lane per (trajectory,
//    step, direction), written as the A and B tiles (chain_linearize_tiles_kernel), or
//    ILQR_LINEARIZE_ANALYTIC, the duals' Jacobians from the tangent of the Newton-Euler pass
//    at fixed q̈ (chain_linearize_analytic_kernel).
//  * the costs as the tiles the recursion reads (launch_tiles_backward, ilqr_tiles.hip);
//    cost_functions.jl's task-space costs with the kinematics composed on the device at every
//    evaluation (ChainTaskK, ilqr_chain_set_task_costs, ilqr_chain_final_cost_quadratize).
//  * a goal per trajectory (ilqr_chain_set_joint_targets: θ*, ilqr_chain_set_task_targets:
//    final_target): the ChainGoalRows instantiations of the cost tiles, the task
//    quadratization and the forward kernels; a handle without rows launches the
//    instantiations it always did.
//  * forward_pass: a 32-lane group per trajectory on the component-parallel Newton-Euler.
//  * f(x, u) alone in fp32 and fp64 (ilqr_chain_dynamics).
#include "ilqr_chain_host.h"
#include "ilqr_fwd_group.h"

#if !defined(ILQR_CHAIN_NJ) || ILQR_CHAIN_NJ < 4 || ILQR_CHAIN_NJ > 7
#error "ilqr_chain_tiles.hip is compiled once per joint count: -DILQR_CHAIN_NJ=4, 5, 6 or 7"
#endif

namespace ilqr {
namespace {

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
template <class X, class... A>
constexpr int pack_count = (0 + ... + (std::is_same_v<A, X> ? 1 : 0));

// Joint-velocity weights (ilqr_chain_set_velocity_weights): ℓ_t += Σ vwᵢ q̇ᵢ², ℓ_f += Σ vfwᵢ q̇ᵢ²
// at T, q̇ᵢ = x[NJ + i], in every cost mode. One more trailing pack type, always the last and
// by value: empty for a handle without weights, whose instantiations, kernel arguments and
// code stay what they were.
template <int NJ>
struct ChainVelK {
  double vw[NJ], vfw[NJ];
};
template <int NJ>
__device__ __forceinline__ const double* goal_rows(const ChainGoalRows& g, const ChainVelK<NJ>&) { return g.rows; }
template <class X, class A0, class... A>
__device__ __forceinline__ const X& pack_get(const A0& a0, const A&... a) {
  if constexpr (std::is_same_v<A0, X>) return a0;
  else return pack_get<X>(a...);
}

// The cost tiles that change with (x, u), the terms chain_backward4_wave forms for two joints
// (immediate_cost_quadratization :81-109, final_cost_quadratization :134-153):
// lx = −2qw(θ* − θ) on the joint rows, lu = 2rw·u, lfx = −2qfw(θ* − θ_N).
// One lane per element: (b, t ≤ T, e < NX + NU), t = T the terminal row.
// Goal: none (θ* = C.tgt) or ChainGoalRows (θ* = row b), then none or ChainVelK: the velocity
// rows, 0 without it, are then lx = 2vw·q̇ and lfx = 2vfw·q̇_N.
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
  // (no local constants here: they would shift the instruction order of the instantiations without weights)
  static_assert(sizeof...(Goal) == pack_count<ChainGoalRows, Goal...> + pack_count<ChainVelK<NJ>, Goal...> &&
                    pack_count<ChainGoalRows, Goal...> <= 1 && pack_count<ChainVelK<NJ>, Goal...> <= 1,
                "Goal: none or ChainGoalRows, then none or ChainVelK");
  if constexpr (pack_count<ChainVelK<NJ>, Goal...> == 1) {  // a velocity element: 2vw·q̇ (2vfw·q̇ at T) where the code below stores 0.0
    if (e >= NJ && e < NX) {
      const ChainVelK<NJ>& W = pack_get<ChainVelK<NJ>>(G...);
      double vw = W.vw[0], vfw = W.vfw[0];
#pragma unroll
      for (int i = 1; i < NJ; ++i)
        if (i == e - NJ) { vw = W.vw[i]; vfw = W.vfw[i]; }
      const double xe = x[((size_t)b * (T + 1) + t) * NX + e];
      if (t == T) lfx[(size_t)b * NX + e] = 2.0 * vfw * xe;
      else lx[((size_t)b * T + t) * NX + e] = 2.0 * vw * xe;
      return;
    }
  }
  if constexpr (pack_count<ChainGoalRows, Goal...> == 1)
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
// Vel: none, or ChainVelK — the velocity diagonals, 0 without it, are then 2vw and 2vfw.
template <int NJ, int NU, class... Vel>
__global__ __launch_bounds__(256) void chain_cost_hessians_kernel(ChainCostK<NJ> C, Vel... W, int B, int T,
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
  static_assert((std::is_same_v<Vel, ChainVelK<NJ>> && ...) && sizeof...(Vel) <= 1, "Vel: none or ChainVelK");
  if constexpr (sizeof...(Vel) == 1) {  // the weight of row r, joint or velocity
    const ChainVelK<NJ>& V = pack_get<ChainVelK<NJ>>(W...);
#pragma unroll
    for (int i = 0; i < NJ; ++i)
      if (NJ + i == r) { qw = V.vw[i]; qfw = V.vfw[i]; }
    if (t == T) {
      lfxx[(size_t)b * NX * NX + e] = r == c ? 2.0 * qfw : 0.0;
    } else {
      const size_t s = (size_t)b * T + t;
      lxx[s * NX * NX + e] = r == c ? 2.0 * qw : 0.0;
      if (e < NU * NU) luu[s * NU * NU + e] = ru == cu ? 2.0 * rw : 0.0;
    }
  } else if (t == T) {
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
// closed form (ChainTask) would carry 3^NJ coefficients here. The constants are ChainTaskK
// (ilqr_chain_model.h: the handle keeps them).
// ---------------------------------------------------------------------------
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
// 3 otherwise; the caller has n ≤ the rows it holds) — then none or ChainVelK: both uses add
// Σ vfwᵢ q̇ᵢ² to the cost, 2vfwᵢq̇ᵢ as the velocity rows of the gradient and 2vfwᵢ on the
// velocity diagonal of the Hessian (still exactly symmetric, the rest of those rows and
// columns exactly 0).
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
  constexpr bool ROWS = pack_count<ChainGoalRows, Goal...> == 1, VEL = pack_count<ChainVelK<NJ>, Goal...> == 1;
  static_assert(sizeof...(Goal) == (ROWS ? 1 : 0) + (VEL ? 1 : 0), "Goal: none or ChainGoalRows, then none or ChainVelK");
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
  if constexpr (VEL) {  // … + Σ vfwᵢ q̇ᵢ²: the velocity rows of ∇ℓ_f and the velocity diagonal of ∇²ℓ_f
    const ChainVelK<NJ>& W = pack_get<ChainVelK<NJ>>(G...);
    double qd[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      qd[i] = xb[NJ + i];
      c = fma(W.vfw[i] * qd[i], qd[i], c);
    }
    if (cost) cost[b] = c;
    if (grad) {
      double* go = grad + (size_t)b * NX;
#pragma unroll
      for (int i = 0; i < NJ; ++i) {
        go[i] = g[i];
        go[NJ + i] = 2.0 * W.vfw[i] * qd[i];
      }
    }
    if (hess) {
      double* ho = hess + (size_t)b * NX * NX;
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          const int lo = i < j ? i : j, hi = i < j ? j : i;
          ho[i * NX + j] = hi < NJ ? H[lo][hi] : (lo == hi ? 2.0 * W.vfw[lo - NJ] : 0.0);
        }
    }
    return;
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

// A tool path (ilqr_chain_set_task_path): the handle's copy of the (batch, T + 1, 3) rows and
// the running weight. While it is set and a task mode is in effect the stage cost is
// ℓ_t = Σū² + w · Σₖ (πₖ(q) − rows[b, t, k])², π the mode's reading of the point
// (chain_task_value); row T is trajectory b's final_target, which the kernels that read a
// goal get as the handle's compact copy of those rows (ChainGoalRows).
struct ChainPath {
  const double* rows;
  double w;
};
__device__ __forceinline__ const ChainPath& path_of(const ChainGoalRows&, const ChainPath& p) { return p; }
__device__ __forceinline__ const double* goal_rows(const ChainGoalRows& g, const ChainPath&) { return g.rows; }
template <int NJ>
__device__ __forceinline__ const ChainPath& path_of(const ChainGoalRows&, const ChainPath& p, const ChainVelK<NJ>&) {
  return p;
}
template <int NJ>
__device__ __forceinline__ const double* goal_rows(const ChainGoalRows& g, const ChainPath&, const ChainVelK<NJ>&) {
  return g.rows;
}

// The per-step tiles of the path cost, one lane per (b, t < T): the quadratization of
// w · Σₖ (πₖ(q) − rows[b, t, k])² at x[b, t] (chain_task_quad_fk on a ChainTaskK whose target
// is the step's row and whose weight is the path's) as the joint rows of lx[b, t] —
// chain_cost_tiles_kernel, which runs before, wrote the velocity rows (0) and lu = 2u — and
// the whole lxx[b, t] tile: i ≤ j computed and mirrored, so exactly symmetric, velocity rows
// and columns exactly 0. Trajectories whose status is not OK are skipped like that kernel's.
// Vel: none, or ChainVelK — the velocity diagonal of lxx[b, t] is then 2vw (the velocity rows
// of lx stay chain_cost_tiles_kernel's).
template <int NJ, class... Vel>
__global__ __launch_bounds__(64) void chain_path_tiles_kernel(ChainK<double, NJ> P, ChainTaskK C, ChainPath path, Vel... W,
                                                              int B, int T, const double* __restrict__ x,
                                                              const int32_t* __restrict__ status,
                                                              double* __restrict__ lx, double* __restrict__ lxx) {
  constexpr int NX = 2 * NJ;
  const size_t bt = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (bt >= (size_t)B * T) return;
  const int b = (int)(bt / T), t = (int)(bt - (size_t)b * T);
  if (status && status[b] != ILQR_TRAJ_OK) return;
  const size_t row = (size_t)b * (T + 1) + t;
  const double* xb = x + row * NX;
  double q[NJ], c, g[NJ], H[NJ][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) q[i] = xb[i];
  ChainTaskK Cp = C;
#pragma unroll
  for (int k = 0; k < 3; ++k) Cp.t[k] = path.rows[row * 3 + k];
  Cp.w = path.w;
  chain_task_quad_fk<NJ>(P, Cp, q, c, g, H);
  double* go = lx + bt * NX;
#pragma unroll
  for (int i = 0; i < NJ; ++i) go[i] = g[i];
  double* ho = lxx + bt * NX * NX;
  static_assert((std::is_same_v<Vel, ChainVelK<NJ>> && ...) && sizeof...(Vel) <= 1, "Vel: none or ChainVelK");
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      if constexpr (sizeof...(Vel) == 1)
        ho[i * NX + j] = hi < NJ ? H[lo][hi] : (lo == hi ? 2.0 * pack_get<ChainVelK<NJ>>(W...).vw[lo - NJ] : 0.0);
      else
        ho[i * NX + j] = hi < NJ ? H[lo][hi] : 0.0;
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
constexpr int CH32_WG = 64;  // two trajectories per workgroup (one wave)
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
// tail, which every lane count leaves (12, 21, 26 and 27 words for 4..7 joints): the lanes
// whose words fall past the record re-read K's first word at every step anyway, so with ROWS
// the first NG of those words read the row instead (stride 0) and the hand-off delivers it
// to the group at stage[N_IN ..) — no register beyond what the shared-goal code holds, which
// at seven joints already fills both register files.
// A tool path (Goal = ChainGoalRows, ChainPath; TASK and ROWS both set, the row being the
// path's row T): every step adds chain_task_value of the step's path row at the point of q̄_t
// to chain_task_stage(ū), every lane of the group on its own copy of x̄_t by the same code,
// as the terminal cost. Step t's row rides in the tail too, three words behind the goal row
// at stage[N_IN + NG ..) with stride 3, prefetched one step ahead with the record. The
// kinematics sit before the RK4 step, so their temporaries are dead at its stages.
// Velocity weights (ChainVelK last in Goal, any mode): every step adds fma(vwᵢ·e, e, lk) in
// joint order after the mode's terms, the terminal cost fma(vfwᵢ·x̄[NJ + i], x̄[NJ + i], lf). With
// TASK e is the raw x̄[NJ + i]; in the joint mode it is x̄[NJ + i] − xtw·x_traj[NJ + i], and the
// NJ velocity words of x_traj ride in the tail as well, behind the goal row at
// stage[N_IN + NG + NP ..) with stride NX, prefetched with the record (the record itself keeps
// its length: N_IN and every offset stay). The weights are read from an LDS copy per group.
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
  constexpr bool PATH = pack_count<ChainPath, Goal...> == 1, VEL = pack_count<ChainVelK<NJ>, Goal...> == 1;
  static_assert(pack_count<ChainGoalRows, Goal...> == (ROWS ? 1 : 0) &&
                    sizeof...(Goal) == (ROWS ? 1 : 0) + (PATH ? 1 : 0) + (VEL ? 1 : 0),
                "Goal: ChainGoalRows with ROWS, else none (the shared-goal instantiations keep their signature)");
  static_assert(!PATH || (TASK && ROWS), "Goal: ChainGoalRows, ChainPath in a task mode with a path");
  constexpr int NX = 2 * NJ, NK = NU * NX;
  constexpr int O_X = NK, O_XT = O_X + NX, O_U = O_XT + NJ, O_D = O_U + NU, N_IN = O_D + NU;
  constexpr int NW = ChainStage<NJ, NU>::WORDS;
  static_assert(N_IN == ChainStage<NJ, NU>::N_IN && N_IN <= ChainStage<NJ, NU>::SIZE && NX + NU <= CH32_LANES,
                "a step's inputs in NW words per lane, x̄ and ū stored by one lane each");
  constexpr int NG = ROWS ? (TASK ? 3 : NJ) : 0, O_G = N_IN;  // the goal row in the stage's tail
  constexpr int NP = PATH ? 3 : 0, O_P = O_G + NG;  // the step's path row behind it
  constexpr int NV = VEL && !TASK ? NJ : 0, O_V = O_P + NP;  // x_traj's velocity rows behind them
  static_assert(N_IN + NG + NP + NV <= ChainStage<NJ, NU>::SIZE,
                "the goal row, the path row and the velocity reference fit the stage's unused tail");
  const int l32 = threadIdx.x & (CH32_LANES - 1);
  // the velocity weights: the group's own LDS copy, read where the step's cost uses them; the
  // cost is pinned before the RK4 stages (below), so they are dead there
  [[maybe_unused]] const ChainVelK<NJ>* W = nullptr;
  if constexpr (VEL) {
    __shared__ ChainVelK<NJ> Ws[CH32_WG / CH32_LANES];
    ChainVelK<NJ>* mine = Ws + threadIdx.x / CH32_LANES;
    static_assert(sizeof(ChainVelK<NJ>) == 2 * NJ * sizeof(double) && 2 * NJ <= CH32_LANES, "one word per lane");
    if (l32 < 2 * NJ)
      reinterpret_cast<double*>(mine)[l32] = reinterpret_cast<const double*>(&pack_get<ChainVelK<NJ>>(G...))[l32];
    wave_lds_fence();
    W = mine;
  }
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
      if constexpr (PATH)
        if (e >= O_P && e < O_P + NP) {
          src[k] = path_of(G...).rows + (size_t)b * (T + 1) * 3 + (e - O_P);
          str[k] = 3;
        }
      if constexpr (NV > 0)
        if (e >= O_V && e < O_V + NV) {
          src[k] = xt0 + NJ + (e - O_V);
          str[k] = NX;
        }
    } else if constexpr (NV > 0) {
      if (e < O_V + NV) {
        src[k] = xt0 + NJ + (e - O_V);
        str[k] = NX;
      }
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
        if constexpr (PATH) {  // … + w Σₖ (πₖ(q̄ₖ) − row_k)², the hand-off left the step's row
          V q[NJ], pw[3];
#pragma unroll
          for (int i = 0; i < NJ; ++i) q[i] = xb[i];
          chain_point_fk<NJ>(P, C, q, pw);
          ChainTaskK Cp = C;
#pragma unroll
          for (int k = 0; k < 3; ++k) Cp.t[k] = stage[O_P + k];
          Cp.w = path_of(G...).w;
          lk = lk + chain_task_value(Cp, pw);
        }
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
      if constexpr (VEL) {  // … + Σ vwᵢ q̇ᵢ², the joint mode's q̇ against x_traj's velocity rows
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
          V e = xb[NJ + i];
          if constexpr (!TASK) e = fma(-xtw, stage[O_V + i], e);
          lk = fma(W->vw[i] * e, e, lk);
        }
      }
      cost += lk;
      if constexpr (VEL) {
        // the step's cost is complete here, before the RK4 stages: left to itself the compiler
        // sinks the whole sum behind chain_rk4_cv32 and keeps the weights and x_traj's velocity
        // words (4·NJ registers) live across every stage
        asm volatile("" : "+v"(cost));
        __builtin_amdgcn_sched_barrier(0);
      }
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
    if constexpr (VEL) {
#pragma unroll
      for (int i = 0; i < NJ; ++i) lf = fma(W->vfw[i] * xb[NJ + i], xb[NJ + i], lf);
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
// … and with velocity weights, with the shared goal or a goal per trajectory
template <int NJ, int NU, bool TASK, bool ROWS>
__device__ __forceinline__ ChainFwdOut<double> chain_forward_group32(
    const ChainK<double, NJ>& P, double* __restrict__ stage, int b, int T, const double* __restrict__ x,
    const double* __restrict__ u, const double* __restrict__ xtraj, const double* __restrict__ dg,
    const double* __restrict__ Kg, double prev_cost, double* __restrict__ xnew, double* __restrict__ unew,
    double* du2_out, const LSParams& ls, const ChainVelK<NJ>& W) {
  static_assert(!TASK && !ROWS, "the joint-space costs with velocity weights");
  return chain_forward_group32<NJ, NU, false, false>(P, stage, b, T, x, u, xtraj, dg, Kg, prev_cost, xnew, unew,
                                                     du2_out, ls, ChainTaskK{}, W);
}
template <int NJ, int NU, bool TASK, bool ROWS>
__device__ __forceinline__ ChainFwdOut<double> chain_forward_group32(
    const ChainK<double, NJ>& P, double* __restrict__ stage, int b, int T, const double* __restrict__ x,
    const double* __restrict__ u, const double* __restrict__ xtraj, const double* __restrict__ dg,
    const double* __restrict__ Kg, double prev_cost, double* __restrict__ xnew, double* __restrict__ unew,
    double* du2_out, const LSParams& ls, const ChainGoalRows& G, const ChainVelK<NJ>& W) {
  static_assert(!TASK && ROWS, "the joint-space costs of a handle with a goal per trajectory and velocity weights");
  return chain_forward_group32<NJ, NU, false, true>(P, stage, b, T, x, u, xtraj, dg, Kg, prev_cost, xnew, unew, du2_out,
                                                    ls, ChainTaskK{}, G, W);
}

// The two forward kernels. TaskK is empty (the joint-space cost) or ChainTaskK (a task mode:
// the TASK instantiation of the group, the task cost's constants one more kernel argument),
// either followed by ChainGoalRows (a goal per trajectory: the ROWS instantiation, the rows'
// pointer one more argument). As a pack it adds nothing to the joint-cost kernels' argument
// list, so every mode keeps the kernel arguments, and with them the code, that each had as a
// kernel written out. A pack in the middle of the list is never deduced: every launch spells
// out <NJ, NU>, <NJ, NU, ChainTaskK>, <NJ, NU, ChainGoalRows>,
// <NJ, NU, ChainTaskK, ChainGoalRows> or <NJ, NU, ChainTaskK, ChainGoalRows, ChainPath> (a tool
// path: the goal rows are then the path's rows T).
// none | ChainTaskK | ChainGoalRows | ChainTaskK, ChainGoalRows | ChainTaskK, ChainGoalRows, ChainPath,
// each followed by none or ChainVelK<NJ> (velocity weights: always the last of the pack)
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
template <>
struct CostPack<ChainTaskK, ChainGoalRows, ChainPath> : std::true_type {};
// … each followed by none or ChainVelK (velocity weights)
template <int NJ>
struct CostPack<ChainVelK<NJ>> : std::true_type {};
template <int NJ>
struct CostPack<ChainTaskK, ChainVelK<NJ>> : std::true_type {};
template <int NJ>
struct CostPack<ChainGoalRows, ChainVelK<NJ>> : std::true_type {};
template <int NJ>
struct CostPack<ChainTaskK, ChainGoalRows, ChainVelK<NJ>> : std::true_type {};
template <int NJ>
struct CostPack<ChainTaskK, ChainGoalRows, ChainPath, ChainVelK<NJ>> : std::true_type {};
template <int NJ, int NU, class... TaskK>
__global__ __launch_bounds__(CH32_WG) void chain_forward32_kernel(
    ChainK<double, NJ> P, TaskK... C, int B, int T, const double* __restrict__ x, const double* __restrict__ u,
    const double* __restrict__ xtraj, const double* __restrict__ d, const double* __restrict__ K,
    const double* __restrict__ prev_cost, double* __restrict__ xnew, double* __restrict__ unew,
    double* __restrict__ new_cost, int32_t* __restrict__ trials, int32_t* __restrict__ status, LSParams ls) {
  static_assert(CostPack<TaskK...>::value, "TaskK: none or ChainTaskK, then none or ChainGoalRows, then none or ChainPath, then none or ChainVelK");
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
  static_assert(CostPack<TaskK...>::value, "TaskK: none or ChainTaskK, then none or ChainGoalRows, then none or ChainPath, then none or ChainVelK");
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

namespace {

// This object's joint count, every joint driven (nu = NJ, fp64): the handle's operations on
// the tiles path — the linearisation and the costs written as tiles,
// launch_tiles_backward(2·NJ, NJ), the 32-lane forward group.
struct ChainTilesOps {
  static constexpr int NJ = ILQR_CHAIN_NJ, NU = NJ, NX = 2 * NJ;
  static_assert(NJ > 3 && NJ + 1 <= 8, "the 32-lane forward group: one role per Newton-Euler pass");
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
  // fn(the extra kernel arguments of a cost pack...): ChainTaskK in a task mode (TASKK: of
  // the kernels that take it as part of the pack), then ChainGoalRows when `rows` is set, then
  // ChainPath while a tool path applies (those kernels only; `rows` is then its rows T). Each
  // launch names its pack from these arguments' types, so a kernel is instantiated for the
  // packs its callers can reach and no other (the comment above CostPack).
  // Last of every pack, ChainVelK while the handle has velocity weights.
  template <bool TASKK, class Fn>
  static hipError_t with_cost_pack(const ilqr_chain_handle* h, const double* rows, Fn&& fn) {
    if (h->tiles.vel_on)
      return with_goal_pack<TASKK>(h, rows, [&](auto... c) { return fn(c..., vel_consts(h)); });
    return with_goal_pack<TASKK>(h, rows, fn);
  }
  static ilqr::ChainVelK<NJ> vel_consts(const ilqr_chain_handle* h) {
    ilqr::ChainVelK<NJ> W{};
    for (int i = 0; i < NJ; ++i) {
      W.vw[i] = h->tiles.v_weight[i];
      W.vfw[i] = h->tiles.vf_weight[i];
    }
    return W;
  }
  template <bool TASKK, class Fn>
  static hipError_t with_goal_pack(const ilqr_chain_handle* h, const double* rows, Fn&& fn) {
    const ilqr::ChainGoalRows g{rows};
    if constexpr (TASKK)
      if (h->task_mode()) {
        if (const double* p = h->tiles.path_rows(true)) return fn(h->tiles.taskk, g, ilqr::ChainPath{p, h->tiles.path_weight});
        return rows ? fn(h->tiles.taskk, g) : fn(h->tiles.taskk);
      }
    return rows ? fn(g) : fn();
  }
  // a goal per trajectory of the cost in effect, or null
  static const double* goal_rows(const ilqr_chain_handle* h) { return h->tiles.goal_rows(h->task_mode()); }

  // lxx, luu, lfxx of the handle's cost in effect: at ilqr_chain_create and at every change
  // of the cost mode (in a task mode h->chain carries q = 0, r = 1, qf = 0: lxx = 0,
  // luu = 2I, and lfxx is rewritten by every backward)
  static hipError_t hessians(ilqr_chain_handle* h) {
    const size_t n = (size_t)h->batch * (h->T + 1) * NX * NX;
    if (h->tiles.vel_on)  // … and the velocity diagonals
      ilqr::chain_cost_hessians_kernel<NJ, NU, ilqr::ChainVelK<NJ>><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
          cost_consts(h->chain), vel_consts(h), h->batch, h->T, h->tiles.lxx, h->tiles.luu, h->tiles.lfxx);
    else
      ilqr::chain_cost_hessians_kernel<NJ, NU><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
          cost_consts(h->chain), h->batch, h->T, h->tiles.lxx, h->tiles.luu, h->tiles.lfxx);
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
  // ilqr_chain_linearize
  static hipError_t linearize_to(ilqr_chain_handle* h, const V* x, const V* u, V* A, V* Bm) {
    return linearize(h, x, u, nullptr, A, Bm);
  }
  // the step's tiles, likewise
  static hipError_t tiles(ilqr_chain_handle* h, const V* x, const V* u, const int32_t* st) {
    const auto& t = h->tiles;
    hipError_t e = linearize(h, x, u, st, t.tA, t.tB);
    if (e != hipSuccess) return e;
    const size_t n = (size_t)h->batch * (h->T + 1) * (NX + NU);
    // θ* per trajectory: the joint mode's rows only (a task mode's weights make lx = 0)
    e = with_cost_pack<false>(h, h->task_mode() ? nullptr : goal_rows(h), [&](auto... c) {
      ilqr::chain_cost_tiles_kernel<NJ, NU, decltype(c)...><<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(
          cost_consts(h->chain), c..., h->batch, h->T, x, u, st, t.lx, t.lu, t.lfx);
      return hipGetLastError();
    });
    if (e != hipSuccess || !h->task_mode()) return e;
    // a task mode: lx = 0 and lu = 2u came from the weights above; with a tool path the joint
    // rows of lx and the lxx tiles from the steps' rows; the terminal tiles from x_N
    if (const double* p = t.path_rows(true)) {
      const size_t np = (size_t)h->batch * h->T;
      if (t.vel_on)
        ilqr::chain_path_tiles_kernel<NJ, ilqr::ChainVelK<NJ>><<<(unsigned)((np + 63) / 64), 64, 0, h->stream>>>(
            chain_consts<V, NJ>(h->chain), t.taskk, ilqr::ChainPath{p, t.path_weight}, vel_consts(h), h->batch, h->T, x,
            st, t.lx, t.lxx);
      else
        ilqr::chain_path_tiles_kernel<NJ><<<(unsigned)((np + 63) / 64), 64, 0, h->stream>>>(
            chain_consts<V, NJ>(h->chain), t.taskk, ilqr::ChainPath{p, t.path_weight}, h->batch, h->T, x, st, t.lx, t.lxx);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return quadratize(h, x + (size_t)h->T * NX, (size_t)(h->T + 1) * NX, h->batch, st, nullptr, t.lfx, t.lfxx);
  }
  // final_cost_quadratization of the cost in effect at n states x[s·stride .. +NX); with a
  // goal per trajectory of that cost, state s against row s (the callers hold n to batch)
  static hipError_t quadratize(ilqr_chain_handle* h, const V* x, size_t stride, int n, const int32_t* st, V* cost,
                               V* grad, V* hess) {
    return with_cost_pack<false>(h, goal_rows(h), [&](auto... c) {
      ilqr::chain_task_quad_kernel<NJ, decltype(c)...><<<(n + 63) / 64, 64, 0, h->stream>>>(
          chain_consts<V, NJ>(h->chain), h->tiles.taskk, c..., h->task_mode() ? 0 : 1, n, x, stride, st, cost, grad,
          hess);
      return hipGetLastError();
    });
  }
  static ilqr::TileParams tile_params(const ilqr_chain_handle* h) {
    const auto& t = h->tiles;
    return ilqr::TileParams{t.tA, t.tB, t.lx, t.lu, t.lxx, nullptr, t.luu, t.lfx, t.lfxx};
  }
  static hipError_t backward(ilqr_chain_handle* h, const V* x, const V* u, V* d, V* K, int32_t* st,
                             double mu) {
    hipError_t e = tiles(h, x, u, nullptr);
    if (e != hipSuccess) return e;
    return ilqr::launch_tiles_backward(NX, NU, tile_params(h), h->batch, h->T, d, K, st ? st : h->tiles.bstatus, mu,
                                       h->stream);
  }
  static int forward_grid(const ilqr_chain_handle* h) {
    return (h->batch * ilqr::CH32_LANES + ilqr::CH32_WG - 1) / ilqr::CH32_WG;
  }
  static hipError_t forward(ilqr_chain_handle* h, const V* x, const V* u, const V* xt, const V* d,
                            const V* K, const V* pc, V* xn, V* un, V* nc, int32_t* tr, int32_t* st,
                            const ilqr::LSParams& ls) {
    const auto P = chain_consts<V, NJ>(h->chain);
    return with_cost_pack<true>(h, goal_rows(h), [&](auto... c) {
      ilqr::chain_forward32_kernel<NJ, NU, decltype(c)...><<<forward_grid(h), ilqr::CH32_WG, 0, h->stream>>>(
          P, c..., h->batch, h->T, x, u, xt, d, K, pc, xn, un, nc, tr, st, ls);
      return hipGetLastError();
    });
  }
  static hipError_t iteration(ilqr_chain_handle* h, const Iter& a, const ilqr::LSParams& ls) {
    hipError_t e = tiles(h, a.x, a.u, a.status);
    if (e != hipSuccess) return e;
    // every trajectory runs the recursion (a stopped one on stale tiles, into the handle's
    // own gains); the forward kernel folds bstatus into the running ones' status
    e = ilqr::launch_tiles_backward(NX, NU, tile_params(h), h->batch, h->T, a.d, a.K, h->tiles.bstatus, ls.mu,
                                    h->stream);
    if (e != hipSuccess) return e;
    const auto P = chain_consts<V, NJ>(h->chain);
    return with_cost_pack<true>(h, goal_rows(h), [&](auto... c) {
      ilqr::chain_iter_forward32_kernel<NJ, NU, decltype(c)...><<<forward_grid(h), ilqr::CH32_WG, 0, h->stream>>>(
          P, c..., h->batch, h->T, a, h->tiles.bstatus, ls);
      return hipGetLastError();
    });
  }
  // ilqr_chain_dynamics, which this shape answers in either dtype
  template <class W>
  static hipError_t dynamics_in(ilqr_chain_handle* h, const W* x, const W* u, W* xo, int n) {
    ilqr::chain_dynamics_kernel<W, NJ, NU><<<(n + 255) / 256, 256, 0, h->stream>>>(chain_consts<W, NJ>(h->chain), n,
                                                                                  x, u, xo);
    return hipGetLastError();
  }
  static hipError_t dynamics(ilqr_chain_handle* h, const double* x, const double* u, double* xo, int n) {
    return dynamics_in(h, x, u, xo, n);
  }
  static hipError_t dynamics_f32(ilqr_chain_handle* h, const float* x, const float* u, float* xo, int n) {
    return dynamics_in(h, x, u, xo, n);
  }
};

}  // namespace

// host data: a constant-initialised const would otherwise be emitted into the code object too
#ifndef __HIP_DEVICE_COMPILE__
#define ILQR_CHAIN_TABLE_(nj) chain_tiles_table_##nj
#define ILQR_CHAIN_TABLE(nj) ILQR_CHAIN_TABLE_(nj)
const ilqr::ChainTilesTable ilqr::ILQR_CHAIN_TABLE(ILQR_CHAIN_NJ) = {
    ChainTilesOps::hessians,  ChainTilesOps::linearize_to, ChainTilesOps::backward,     ChainTilesOps::forward,
    ChainTilesOps::iteration, ChainTilesOps::quadratize,   ChainTilesOps::dynamics,     ChainTilesOps::dynamics_f32};
#endif
