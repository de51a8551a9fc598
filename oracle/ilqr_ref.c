/*
 * ilqr_ref.c — C restatement of aabouman/iLQR.jl's hot path (LQ, 2-link arm, caller tiles and RBD chain families)
 * — TEST INFRASTRUCTURE ONLY (checker for the GPU parity tests and the
 * bench's cpu_baseline leg; never linked into the product).
 *
 * The reference is pure Julia (not buildable here: no Julia toolchain), so this
 * is a line-by-line restatement of its algorithm with the LQ callbacks
 *   dynamicsf(x,u) = A x + B u, immediate_cost(x,u) = xᵀQx + uᵀRu, final_cost(x) = xᵀQf x
 * whose ForwardDiff derivatives are exact:
 *   linearize_dynamics            (src/backward_pass.jl:25-40)   → A, B
 *   immediate_cost_quadratization (src/backward_pass.jl:81-109)  → 𝐪=(Q+Qᵀ)x, 𝐫=(R+Rᵀ)u, 𝐐=Q+Qᵀ, 𝐏=0, 𝐑=R+Rᵀ
 *   final_cost_quadratization     (src/backward_pass.jl:134-153) → (Qf+Qfᵀ)x, Qf+Qfᵀ
 *   optimal_controller_param      (src/backward_pass.jl:177-186)
 *   feedback_parameters           (src/backward_pass.jl:207-218) H_reg = H + 0.01 I, `\` = LU w/ partial pivoting
 *   step_back                     (src/backward_pass.jl:262-273) unregularised H
 *   backward_pass                 (src/backward_pass.jl:324-357)
 *   forward_pass                  (src/forward_pass.jl:55-93)    α halving, α on δu only
 *   total_cost                    (src/forward_pass.jl:182-196)  sequential sum, ℓ_f on raw x̄_N
 *   fit                           (src/forward_pass.jl:148-179)  prev_cost=Inf, break before update
 * The same algorithm runs the 2-link arm of test/2_link_example (oracle_tl_*),
 * its derivatives by dual-number forward-mode AD.
 * The reference's unbounded line search is capped at max_trials (status 3).
 * Layout: the ABI's (include/ilqr.h) row-major, trajectory-slowest arrays.
 * OpenMP parallelises over independent trajectories only.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define NMAX 32
#define MMAX 16

/* y[r] = M[r][:] x   (M row-major r×c) */
static void matvec(int r, int c, const double* M, const double* x, double* y) {
  for (int i = 0; i < r; ++i) {
    double s = 0.0;
    for (int k = 0; k < c; ++k) s += M[i * c + k] * x[k];
    y[i] = s;
  }
}
/* y = Mᵀ x  (M row-major r×c, y length c) */
static void matTvec(int r, int c, const double* M, const double* x, double* y) {
  for (int j = 0; j < c; ++j) {
    double s = 0.0;
    for (int k = 0; k < r; ++k) s += M[k * c + j] * x[k];
    y[j] = s;
  }
}
/* C = A(r×k) B(k×c) */
static void matmul(int r, int k, int c, const double* A, const double* B, double* C) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) {
      double s = 0.0;
      for (int p = 0; p < k; ++p) s += A[i * k + p] * B[p * c + j];
      C[i * c + j] = s;
    }
}
/* C = Aᵀ(A is k×r) B(k×c) */
static void matTmul(int k, int r, int c, const double* A, const double* B, double* C) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) {
      double s = 0.0;
      for (int p = 0; p < k; ++p) s += A[p * r + i] * B[p * c + j];
      C[i * c + j] = s;
    }
}

/* Solve M X = Y in place (M m×m, Y m×c), LU with partial pivoting. Returns 0 if singular. */
static int lu_solve(int m, double* M, int c, double* Y) {
  int piv[MMAX];
  for (int k = 0; k < m; ++k) {
    int p = k;
    double best = fabs(M[k * m + k]);
    for (int i = k + 1; i < m; ++i)
      if (fabs(M[i * m + k]) > best) { best = fabs(M[i * m + k]); p = i; }
    piv[k] = p;
    if (best == 0.0) return 0;
    if (p != k) {
      for (int j = 0; j < m; ++j) { double t = M[k * m + j]; M[k * m + j] = M[p * m + j]; M[p * m + j] = t; }
      for (int j = 0; j < c; ++j) { double t = Y[k * c + j]; Y[k * c + j] = Y[p * c + j]; Y[p * c + j] = t; }
    }
    for (int i = k + 1; i < m; ++i) {
      const double f = M[i * m + k] / M[k * m + k];
      M[i * m + k] = f;
      for (int j = k + 1; j < m; ++j) M[i * m + j] -= f * M[k * m + j];
      for (int j = 0; j < c; ++j) Y[i * c + j] -= f * Y[k * c + j];
    }
  }
  for (int i = m - 1; i >= 0; --i)
    for (int j = 0; j < c; ++j) {
      double s = Y[i * c + j];
      for (int p = i + 1; p < m; ++p) s -= M[i * m + p] * Y[p * c + j];
      Y[i * c + j] = s / M[i * m + i];
    }
  (void)piv;
  return 1;
}

/* One trajectory's problem: the reference's three callbacks (dynamicsf,
 * immediate_cost, final_cost) and the derivatives ForwardDiff takes of them
 * (linearize_dynamics / immediate_cost_quadratization / final_cost_quadratization). */
typedef struct prob_s prob_t;
struct prob_s {
  int n, m, T;
  const double *A, *B, *Q, *R, *Qf; /* LQ family: this trajectory's instance */
  const double* const* tiles;        /* TILES family: caller-supplied derivatives */
  void (*lin)(const prob_t*, int t, const double* x, const double* u, double* A, double* B);
  /* 𝐪 (n), 𝐫 (m), 𝐐 (n×n), 𝐏 (m×n), 𝐑 (m×m) */
  void (*quad)(const prob_t*, int t, const double* x, const double* u, double* qv, double* r,
               double* Q, double* P, double* R);
  void (*fquad)(const prob_t*, const double* x, double* s, double* S);
  void (*dyn)(const prob_t*, const double* x, const double* u, double* xn);
  double (*cost)(const prob_t*, const double* x, const double* u);
  double (*fcost)(const prob_t*, const double* x);
  const void* ext; /* CHAIN family: the chain's constants (chain_t) */
};

/* -- LQ family: f = Ax + Bu, ℓ = xᵀQx + uᵀRu, ℓ_f = xᵀQf x (exact derivatives) -- */
static void lq_lin(const prob_t* P, int t, const double* x, const double* u, double* A, double* B) {
  (void)t; (void)x; (void)u;
  memcpy(A, P->A, sizeof(double) * P->n * P->n);
  memcpy(B, P->B, sizeof(double) * P->n * P->m);
}
static void lq_quad(const prob_t* P, int t, const double* x, const double* u, double* qv,
                    double* r, double* Qs, double* Pm, double* Rs) {
  (void)t;
  const int n = P->n, m = P->m;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Qs[i * n + j] = P->Q[i * n + j] + P->Q[j * n + i];
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) Rs[i * m + j] = P->R[i * m + j] + P->R[j * m + i];
  memset(Pm, 0, sizeof(double) * m * n);
  matvec(n, n, Qs, x, qv);
  matvec(m, m, Rs, u, r);
}
static void lq_fquad(const prob_t* P, const double* x, double* s, double* S) {
  const int n = P->n;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) S[i * n + j] = P->Qf[i * n + j] + P->Qf[j * n + i];
  matvec(n, n, S, x, s);
}
static void lq_dyn(const prob_t* P, const double* x, const double* u, double* xn) {
  double t1[NMAX], t2[NMAX];
  matvec(P->n, P->n, P->A, x, t1);
  matvec(P->n, P->m, P->B, u, t2);
  for (int i = 0; i < P->n; ++i) xn[i] = t1[i] + t2[i];
}
static double lq_cost(const prob_t* P, const double* x, const double* u) {
  double t[NMAX];
  double c = 0.0;
  matvec(P->n, P->n, P->Q, x, t);
  for (int i = 0; i < P->n; ++i) c += x[i] * t[i];
  matvec(P->m, P->m, P->R, u, t);
  double cu = 0.0;
  for (int i = 0; i < P->m; ++i) cu += u[i] * t[i];
  return c + cu;
}
static double lq_fcost(const prob_t* P, const double* x) {
  double t[NMAX];
  double c = 0.0;
  matvec(P->n, P->n, P->Qf, x, t);
  for (int i = 0; i < P->n; ++i) c += x[i] * t[i];
  return c;
}

/* -- 2-link arm: test/2_link_example/2_link_helper_functions.jl:1-108 ----------------
 * Restates oracle/ilqr_oracle.py's TwoLink (literal, quirks included): RK4 of
 * [θ̇; −(M⁻¹C)θ̇ + M⁻¹u] with the script's CoriolisMatrix (k = 2 term only), the
 * 2×2 inverse by cofactors (ilqr_oracle._inv2). linearize_dynamics is forward-mode
 * AD with the 6 directions (x, u) carried together — ForwardDiff's arithmetic. */
typedef struct { double v, d[6]; } dual6;
static dual6 dc(double v) { dual6 r; r.v = v; for (int i = 0; i < 6; ++i) r.d[i] = 0.0; return r; }
static dual6 dadd(dual6 a, dual6 b) { dual6 r; r.v = a.v + b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
static dual6 dsub(dual6 a, dual6 b) { dual6 r; r.v = a.v - b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
static dual6 dneg(dual6 a) { dual6 r; r.v = -a.v; for (int i = 0; i < 6; ++i) r.d[i] = -a.d[i]; return r; }
static dual6 dmul(dual6 a, dual6 b) { dual6 r; r.v = a.v * b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
static dual6 dscale(double a, dual6 b) { dual6 r; r.v = a * b.v; for (int i = 0; i < 6; ++i) r.d[i] = a * b.d[i]; return r; }
static dual6 ddiv(dual6 a, dual6 b) {
  dual6 r; r.v = a.v / b.v;
  for (int i = 0; i < 6; ++i) r.d[i] = (a.d[i] * b.v - a.v * b.d[i]) / (b.v * b.v);
  return r;
}
static dual6 dsin(dual6 a) { dual6 r; r.v = sin(a.v); const double c = cos(a.v); for (int i = 0; i < 6; ++i) r.d[i] = c * a.d[i]; return r; }
static dual6 dcos(dual6 a) { dual6 r; r.v = cos(a.v); const double s = -sin(a.v); for (int i = 0; i < 6; ++i) r.d[i] = s * a.d[i]; return r; }

typedef struct { double alpha, beta, delta, dt, tgt0, tgt1; } tl_consts;
static tl_consts TL;
static void tl_init(void) {
  static int done = 0;
  if (done) return;
  const double l1 = sqrt(2.) / 2., l2 = sqrt(2.) / 2., r2 = 0.5 * l2, r1 = 0.5 * l1;
  const double m1 = 1.0, m2 = 1.0;
  const double Iz1 = 1.0 / 12.0 * m1 * (l1 * l1), Iz2 = 1.0 / 12.0 * m2 * (l2 * l2);
  TL.alpha = Iz1 + Iz2 + m1 * (r1 * r1) + m2 * (l1 * l1 + r2 * r2);   /* :11 */
  TL.beta = m2 * l1 * r2;                                              /* :12 */
  TL.delta = Iz2 + m2 * (r2 * r2);                                     /* :13 */
  TL.dt = 0.01;                                                        /* :14 */
  const double x = 0.6, y = -0.5;                                      /* :16 */
  const double q2 = acos((x * x + y * y - l1 * l1 - l2 * l2) / (2 * l1 * l2));  /* :22-23 */
  TL.tgt0 = atan2(y, x) - atan2(l2 * sin(q2), l1 + l2 * cos(q2));
  TL.tgt1 = q2;
  done = 1;
}

/* test-only: another target_tool_loc (2_link_helper_functions.jl:16) — the reference's
 * shipped animations of the other quadrants (tests/test_reference_gifs.py); the script's
 * own (0.6, −0.5) is the default. Not thread-safe against running fits. */
void oracle_tl_set_target(double x, double y) {
  tl_init();
  const double l1 = sqrt(2.) / 2., l2 = sqrt(2.) / 2.;
  const double q2 = acos((x * x + y * y - l1 * l1 - l2 * l2) / (2 * l1 * l2));  /* :22-23 */
  TL.tgt0 = atan2(y, x) - atan2(l2 * sin(q2), l1 + l2 * cos(q2));
  TL.tgt1 = q2;
}

/* test-only (tests/test_reference_gifs.py::test_gif_pin_sensitivity): 1 = the textbook
 * Coriolis matrix (Christoffel symbols summed over every k) in place of the script's
 * CoriolisMatrix, whose `for k in length(θ)` (:42-44) leaves ½·θ̇₂·∂M/∂θ₂:
 * C = [−βs₂θ̇₂, −βs₂(θ̇₁+θ̇₂); βs₂θ̇₁, 0] against [−βs₂θ̇₂, −½βs₂θ̇₂; −½βs₂θ̇₂, 0]. */
static int TL_PHYSICAL_CORIOLIS = 0;
void oracle_tl_set_physical_coriolis(int on) { TL_PHYSICAL_CORIOLIS = on; }

static void tl_cd_dual_tail(const dual6* x, const dual6* u, dual6* xd, dual6 m00, dual6 m01, dual6 c00,
                            dual6 c01, dual6 c10, dual6 c11);
/* continuous_dynamics (:51-69) on duals */
static void tl_cd_dual(const dual6* x, const dual6* u, dual6* xd) {
  const dual6 c2 = dcos(x[1]), s2 = dsin(x[1]);
  const dual6 m00 = dadd(dc(TL.alpha), dscale(2 * TL.beta, c2));
  const dual6 m01 = dadd(dc(TL.delta), dscale(TL.beta, c2));
  const dual6 dm00 = dscale(2 * TL.beta, dneg(s2)), dm01 = dscale(TL.beta, dneg(s2));
  const dual6 zero = dc(0.0);
  /* C[i,j] = ½(∇M[k,i,j] + ∇M[j,i,k] − ∇M[i,k,j])·θ̇[k], k = 2 only (:42-44) */
  const dual6 c00 = dmul(dscale(0.5, dsub(dadd(zero, dm00), zero)), x[3]);
  const dual6 c01 = dmul(dscale(0.5, dsub(dadd(dm01, dm01), dm01)), x[3]);
  const dual6 c10 = dmul(dscale(0.5, dsub(dadd(zero, dm01), zero)), x[3]);
  const dual6 c11 = dmul(dscale(0.5, dsub(dadd(zero, zero), zero)), x[3]);
  if (TL_PHYSICAL_CORIOLIS) {
    const dual6 p01 = dmul(dm01, dadd(x[2], x[3])), p10 = dneg(dmul(dm01, x[2]));
    tl_cd_dual_tail(x, u, xd, m00, m01, c00, p01, p10, zero);
    return;
  }
  tl_cd_dual_tail(x, u, xd, m00, m01, c00, c01, c10, c11);
}
static void tl_cd_dual_tail(const dual6* x, const dual6* u, dual6* xd, dual6 m00, dual6 m01, dual6 c00,
                            dual6 c01, dual6 c10, dual6 c11) {
  const dual6 det = dsub(dmul(m00, dc(TL.delta)), dmul(m01, m01));
  const dual6 i00 = ddiv(dc(TL.delta), det), i01 = ddiv(dneg(m01), det);
  const dual6 i10 = ddiv(dneg(m01), det), i11 = ddiv(m00, det);
  const dual6 mc00 = dadd(dmul(i00, c00), dmul(i01, c10)), mc01 = dadd(dmul(i00, c01), dmul(i01, c11));
  const dual6 mc10 = dadd(dmul(i10, c00), dmul(i11, c10)), mc11 = dadd(dmul(i10, c01), dmul(i11, c11));
  xd[0] = x[2];
  xd[1] = x[3];
  xd[2] = dadd(dneg(dadd(dmul(mc00, x[2]), dmul(mc01, x[3]))), dadd(dmul(i00, u[0]), dmul(i01, u[1])));
  xd[3] = dadd(dneg(dadd(dmul(mc10, x[2]), dmul(mc11, x[3]))), dadd(dmul(i10, u[0]), dmul(i11, u[1])));
}
/* the same on doubles (forward rollout) */
static void tl_cd(const double* x, const double* u, double* xd) {
  const double c2 = cos(x[1]), s2 = sin(x[1]);
  const double m00 = TL.alpha + 2 * TL.beta * c2, m01 = TL.delta + TL.beta * c2;
  const double dm00 = 2 * TL.beta * -s2, dm01 = TL.beta * -s2;
  const double c00 = 0.5 * dm00 * x[3], c01 = 0.5 * ((dm01 + dm01) - dm01) * x[3];
  double c10 = 0.5 * dm01 * x[3], c11 = 0.0 * x[3];
  const double c01p = TL_PHYSICAL_CORIOLIS ? dm01 * (x[2] + x[3]) : c01;
  if (TL_PHYSICAL_CORIOLIS) { c10 = -(dm01 * x[2]); c11 = 0.0; }
  const double det = m00 * TL.delta - m01 * m01;
  const double i00 = TL.delta / det, i01 = -m01 / det, i10 = -m01 / det, i11 = m00 / det;
  const double mc00 = i00 * c00 + i01 * c10, mc01 = i00 * c01p + i01 * c11;
  const double mc10 = i10 * c00 + i11 * c10, mc11 = i10 * c01p + i11 * c11;
  xd[0] = x[2];
  xd[1] = x[3];
  xd[2] = -(mc00 * x[2] + mc01 * x[3]) + (i00 * u[0] + i01 * u[1]);
  xd[3] = -(mc10 * x[2] + mc11 * x[3]) + (i10 * u[0] + i11 * u[1]);
}
/* RK4 (:71-78) */
static void tl_rk4(const double* x, const double* u, double* xn) {
  double k1[4], k2[4], k3[4], k4[4], y[4];
  tl_cd(x, u, k1);
  for (int i = 0; i < 4; ++i) { k1[i] *= TL.dt; y[i] = x[i] + k1[i] / 2; }
  tl_cd(y, u, k2);
  for (int i = 0; i < 4; ++i) { k2[i] *= TL.dt; y[i] = x[i] + k2[i] / 2; }
  tl_cd(y, u, k3);
  for (int i = 0; i < 4; ++i) { k3[i] *= TL.dt; y[i] = x[i] + k3[i]; }
  tl_cd(y, u, k4);
  for (int i = 0; i < 4; ++i) { k4[i] *= TL.dt; xn[i] = x[i] + (1.0 / 6.0) * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]); }
}
static void tl_rk4_dual(const dual6* x, const dual6* u, dual6* xn) {
  dual6 k1[4], k2[4], k3[4], k4[4], y[4];
  tl_cd_dual(x, u, k1);
  for (int i = 0; i < 4; ++i) { k1[i] = dscale(TL.dt, k1[i]); y[i] = dadd(x[i], dscale(0.5, k1[i])); }
  tl_cd_dual(y, u, k2);
  for (int i = 0; i < 4; ++i) { k2[i] = dscale(TL.dt, k2[i]); y[i] = dadd(x[i], dscale(0.5, k2[i])); }
  tl_cd_dual(y, u, k3);
  for (int i = 0; i < 4; ++i) { k3[i] = dscale(TL.dt, k3[i]); y[i] = dadd(x[i], k3[i]); }
  tl_cd_dual(y, u, k4);
  for (int i = 0; i < 4; ++i) {
    k4[i] = dscale(TL.dt, k4[i]);
    xn[i] = dadd(x[i], dscale(1.0 / 6.0, dadd(dadd(dadd(k1[i], dscale(2, k2[i])), dscale(2, k3[i])), k4[i])));
  }
}
static void tl_lin(const prob_t* P, int t, const double* x, const double* u, double* A, double* B) {
  (void)P; (void)t;
  dual6 xs[4], us[2], out[4];
  for (int i = 0; i < 4; ++i) { xs[i] = dc(x[i]); xs[i].d[i] = 1.0; }
  for (int i = 0; i < 2; ++i) { us[i] = dc(u[i]); us[i].d[4 + i] = 1.0; }
  tl_rk4_dual(xs, us, out);
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 4; ++k) A[i * 4 + k] = out[i].d[k];
    for (int k = 0; k < 2; ++k) B[i * 2 + k] = out[i].d[4 + k];
  }
}
/* ℓ = Σ(θ*−θ)²·1 + Σu²·1 (:82-97): exact gradient/Hessian */
static void tl_quad(const prob_t* P, int t, const double* x, const double* u, double* qv,
                    double* r, double* Q, double* Pm, double* R) {
  (void)P; (void)t;
  memset(Q, 0, sizeof(double) * 16);
  memset(Pm, 0, sizeof(double) * 8);
  memset(R, 0, sizeof(double) * 4);
  qv[0] = 2 * (TL.tgt0 - x[0]) * -1.0;
  qv[1] = 2 * (TL.tgt1 - x[1]) * -1.0;
  qv[2] = qv[3] = 0.0;
  Q[0] = Q[5] = 2.0;
  r[0] = 2 * u[0];
  r[1] = 2 * u[1];
  R[0] = R[3] = 2.0;
}
static void tl_fquad(const prob_t* P, const double* x, double* s, double* S) {
  (void)P;
  memset(S, 0, sizeof(double) * 16);
  s[0] = 2 * (TL.tgt0 - x[0]) * -1.0;
  s[1] = 2 * (TL.tgt1 - x[1]) * -1.0;
  s[2] = s[3] = 0.0;
  S[0] = S[5] = 2.0;
}
static void tl_dyn(const prob_t* P, const double* x, const double* u, double* xn) { (void)P; tl_rk4(x, u, xn); }
static double tl_cost(const prob_t* P, const double* x, const double* u) {
  (void)P;
  const double e0 = TL.tgt0 - x[0], e1 = TL.tgt1 - x[1];
  return (e0 * e0 + e1 * e1) * 1.0 + (u[0] * u[0] + u[1] * u[1]) * 1.0;
}
static double tl_fcost(const prob_t* P, const double* x) {
  (void)P;
  const double e0 = TL.tgt0 - x[0], e1 = TL.tgt1 - x[1];
  return (e0 * e0 + e1 * e1) * 1.0;
}
/* the nu = 1 variant f(x, [u₁, 0]) (BASELINE.json configs 1-2; build-defined, see
 * oracle/ilqr_oracle.py TwoLink.dynamicsf_nu1): the second torque a constant 0, its
 * dual direction absent */
static void tl_lin1(const prob_t* P, int t, const double* x, const double* u, double* A, double* B) {
  (void)P; (void)t;
  dual6 xs[4], us[2], out[4];
  for (int i = 0; i < 4; ++i) { xs[i] = dc(x[i]); xs[i].d[i] = 1.0; }
  us[0] = dc(u[0]);
  us[0].d[4] = 1.0;
  us[1] = dc(0.0);
  tl_rk4_dual(xs, us, out);
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 4; ++k) A[i * 4 + k] = out[i].d[k];
    B[i] = out[i].d[4];
  }
}
static void tl_quad1(const prob_t* P, int t, const double* x, const double* u, double* qv,
                     double* r, double* Q, double* Pm, double* R) {
  (void)P; (void)t;
  memset(Q, 0, sizeof(double) * 16);
  memset(Pm, 0, sizeof(double) * 4);
  qv[0] = 2 * (TL.tgt0 - x[0]) * -1.0;
  qv[1] = 2 * (TL.tgt1 - x[1]) * -1.0;
  qv[2] = qv[3] = 0.0;
  Q[0] = Q[5] = 2.0;
  r[0] = 2 * u[0];
  R[0] = 2.0;
}
static void tl_dyn1(const prob_t* P, const double* x, const double* u, double* xn) {
  (void)P;
  const double u2[2] = {u[0], 0.0};
  tl_rk4(x, u2, xn);
}
static double tl_cost1(const prob_t* P, const double* x, const double* u) {
  (void)P;
  const double e0 = TL.tgt0 - x[0], e1 = TL.tgt1 - x[1];
  return (e0 * e0 + e1 * e1) * 1.0 + (u[0] * u[0]) * 1.0;
}
static prob_t tl_problem(int T, int nu) {
  tl_init();
  prob_t P = {4, 2, T, NULL, NULL, NULL, NULL, NULL, NULL, tl_lin, tl_quad, tl_fquad, tl_dyn, tl_cost, tl_fcost};
  prob_t P1 = {4, 1, T, NULL, NULL, NULL, NULL, NULL, NULL, tl_lin1, tl_quad1, tl_fquad, tl_dyn1, tl_cost1, tl_fcost};
  return nu == 1 ? P1 : P;
}

/* -- TILES family: the derivative calls' results supplied per step by the caller --
 * tiles[0..8] = A (T,n,n), B (T,n,m), lx (T,n), lu (T,m), lxx (T,n,n), lux (T,m,n) or
 * NULL, luu (T,m,m), lfx (n), lfxx (n,n) of this trajectory. */
static void tiles_lin(const prob_t* P, int t, const double* x, const double* u, double* A, double* B) {
  (void)x; (void)u;
  const int n = P->n, m = P->m;
  memcpy(A, P->tiles[0] + (size_t)t * n * n, sizeof(double) * n * n);
  memcpy(B, P->tiles[1] + (size_t)t * n * m, sizeof(double) * n * m);
}
static void tiles_quad(const prob_t* P, int t, const double* x, const double* u, double* qv,
                       double* r, double* Q, double* Pm, double* R) {
  (void)x; (void)u;
  const int n = P->n, m = P->m;
  memcpy(qv, P->tiles[2] + (size_t)t * n, sizeof(double) * n);
  memcpy(r, P->tiles[3] + (size_t)t * m, sizeof(double) * m);
  memcpy(Q, P->tiles[4] + (size_t)t * n * n, sizeof(double) * n * n);
  if (P->tiles[5]) memcpy(Pm, P->tiles[5] + (size_t)t * m * n, sizeof(double) * m * n);
  else memset(Pm, 0, sizeof(double) * m * n);
  memcpy(R, P->tiles[6] + (size_t)t * m * m, sizeof(double) * m * m);
}
static void tiles_fquad(const prob_t* P, const double* x, double* s, double* S) {
  (void)x;
  memcpy(s, P->tiles[7], sizeof(double) * P->n);
  memcpy(S, P->tiles[8], sizeof(double) * P->n * P->n);
}

/* backward_pass (backward_pass.jl:324-357) for one trajectory. Returns 1 if NaN. */
static int backward_one(const prob_t* P, const double* x, const double* u, double mu, int sym,
                        double* d, double* K) {
  const int n = P->n, m = P->m, T = P->T;
  double S[NMAX * NMAX], s[NMAX], Qs[NMAX * NMAX], Rs[MMAX * MMAX], Pm[MMAX * NMAX];
  double A[NMAX * NMAX], Bm[NMAX * MMAX];
  double qv[NMAX], r[MMAX], g[MMAX], G[MMAX * NMAX], H[MMAX * MMAX], Hreg[MMAX * MMAX];
  double BtS[MMAX * NMAX], AtS[NMAX * NMAX], t1[NMAX * NMAX], t2[NMAX], du[MMAX], Ki[MMAX * NMAX];
  double HK[MMAX * NMAX], Hdu[MMAX], Snew[NMAX * NMAX], snew[NMAX];
  int nan = 0;
  /* final_cost_quadratization (:134-153) */
  P->fquad(P, x + (size_t)T * n, s, S);
  for (int t = T - 1; t >= 0; --t) { /* :339 */
    const double* xt = x + (size_t)t * n;
    const double* ut = u + (size_t)t * m;
    P->lin(P, t, xt, ut, A, Bm);              /* linearize_dynamics (:25-40) */
    P->quad(P, t, xt, ut, qv, r, Qs, Pm, Rs);  /* immediate_cost_quadratization (:81-109) */
    /* optimal_controller_param (:177-186) */
    matTvec(n, m, Bm, s, g);                   /* Bᵀ s */
    for (int i = 0; i < m; ++i) g[i] += r[i];  /* g = r + Bᵀ s */
    matTmul(n, m, n, Bm, S, BtS);              /* Bᵀ S */
    matmul(m, n, n, BtS, A, G);                /* (BᵀS)A */
    for (int i = 0; i < m * n; ++i) G[i] += Pm[i]; /* G = P + (BᵀS)A */
    matmul(m, n, m, BtS, Bm, H);               /* (BᵀS)B */
    for (int i = 0; i < m * m; ++i) H[i] += Rs[i];
    /* feedback_parameters (:207-218) */
    memcpy(Hreg, H, sizeof(double) * m * m);
    for (int i = 0; i < m; ++i) Hreg[i * m + i] += mu;
    for (int i = 0; i < m; ++i) du[i] = -g[i];
    for (int i = 0; i < m * n; ++i) Ki[i] = -G[i];
    {
      double Hc[MMAX * MMAX];
      memcpy(Hc, Hreg, sizeof(Hc[0]) * m * m);
      if (!lu_solve(m, Hc, 1, du)) nan = 1;
      memcpy(Hc, Hreg, sizeof(Hc[0]) * m * m);
      if (!lu_solve(m, Hc, n, Ki)) nan = 1;
    }
    for (int i = 0; i < m; ++i) d[(size_t)t * m + i] = du[i];
    for (int i = 0; i < m * n; ++i) K[(size_t)t * m * n + i] = Ki[i];
    /* step_back (:262-273), unregularised H */
    matvec(m, m, H, du, Hdu);
    matTvec(n, n, A, s, snew);                  /* Aᵀ s' */
    for (int i = 0; i < n; ++i) snew[i] += qv[i];
    matTvec(m, n, Ki, Hdu, t2);                 /* Kᵀ H δu */
    for (int i = 0; i < n; ++i) snew[i] += t2[i];
    matTvec(m, n, Ki, g, t2);                   /* Kᵀ g */
    for (int i = 0; i < n; ++i) snew[i] += t2[i];
    matTvec(m, n, G, du, t2);                   /* Gᵀ δu */
    for (int i = 0; i < n; ++i) snew[i] += t2[i];
    matTmul(n, n, n, A, S, AtS);                /* Aᵀ S' */
    matmul(n, n, n, AtS, A, Snew);              /* Aᵀ S' A */
    for (int i = 0; i < n * n; ++i) Snew[i] += Qs[i];
    matmul(m, m, n, H, Ki, HK);
    matTmul(m, n, n, Ki, HK, t1);               /* Kᵀ H K */
    for (int i = 0; i < n * n; ++i) Snew[i] += t1[i];
    matTmul(m, n, n, Ki, G, t1);                /* Kᵀ G */
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) Snew[i * n + j] += t1[i * n + j] + t1[j * n + i]; /* + Gᵀ K */
    if (sym) /* (S+Sᵀ)/2: identity in exact arithmetic, see ilqr_oracle.backward_pass */
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) {
          const double a = 0.5 * (Snew[i * n + j] + Snew[j * n + i]);
          Snew[i * n + j] = a;
          Snew[j * n + i] = a;
        }
    memcpy(S, Snew, sizeof(double) * n * n);
    memcpy(s, snew, sizeof(double) * n);
  }
  for (int i = 0; i < T * m; ++i) nan |= isnan(d[i]);
  for (int i = 0; i < T * m * n; ++i) nan |= isnan(K[i]);
  return nan;
}

/* forward_pass (forward_pass.jl:55-93). Returns trials (>0 accepted, <0 exhausted). gap_out (may
 * be NULL): the closest any trial's cost came to prev_cost, relative to it (Inf for an infinite
 * prev_cost) — how far the search's decisions were from flipping. */
static int forward_one(const prob_t* P, const double* x, const double* u, const double* xtraj,
                       const double* d, const double* K, double prev_cost, double* xb,
                       double* ub, double* cost_out, int max_trials, double alpha0,
                       double shrink, double* gap_out) {
  const int n = P->n, m = P->m, T = P->T;
  double alpha = alpha0;
  double dx[NMAX], e[NMAX], Kdx[MMAX];
  double new_cost = 0.0, gap = INFINITY;
  if (gap_out) *gap_out = gap;
  for (int trial = 1; trial <= max_trials; ++trial) {
    memcpy(xb, x, sizeof(double) * n); /* :65 */
    for (int k = 0; k < T; ++k) {      /* :71 */
      for (int i = 0; i < n; ++i) dx[i] = xb[(size_t)k * n + i] - x[(size_t)k * n + i];
      matvec(m, n, K + (size_t)k * m * n, dx, Kdx);
      for (int i = 0; i < m; ++i)      /* :73 */
        ub[(size_t)k * m + i] = (u[(size_t)k * m + i] + alpha * d[(size_t)k * m + i]) + Kdx[i];
      P->dyn(P, xb + (size_t)k * n, ub + (size_t)k * m, xb + (size_t)(k + 1) * n); /* :74 */
    }
    /* total_cost (:185-193) */
    double acc = 0.0;
    for (int k = 0; k < T; ++k) {
      for (int i = 0; i < n; ++i) e[i] = xb[(size_t)k * n + i] - (xtraj ? xtraj[(size_t)k * n + i] : 0.0);
      acc += P->cost(P, e, ub + (size_t)k * m);
    }
    acc += P->fcost(P, xb + (size_t)T * n);
    new_cost = acc;
    *cost_out = new_cost;
    if (gap_out && isfinite(prev_cost) && fabs(prev_cost - new_cost) / fabs(prev_cost) < gap)
      *gap_out = gap = fabs(prev_cost - new_cost) / fabs(prev_cost);
    if (prev_cost - new_cost > 0) return trial; /* :77-80 */
    alpha *= shrink;                           /* :82 α /= 2 (α *= shrink: the header's rule) */
  }
  return -max_trials;
}

/* -- RBD fixed-base serial chain (test/RBD_2_link_example, BASELINE config 5) ---------
 * Restates oracle/rbd.py's ChainModel / ChainCost (the numpy oracle of the device's
 * ILQR_PROBLEM_CHAIN): recursive Newton-Euler for the bias, M's columns by unit
 * accelerations without gravity, Gaussian elimination, RK4 with dt; linearised by
 * central differences h = ε^⅓·max(1, |z_k|) divided by the step actually taken (the
 * device's ILQR_LINEARIZE_CENTRAL_FD); cost Σ qwᵢ(θ*ᵢ−θᵢ)² + Σ rwₖuₖ², final
 * Σ qfwᵢ(θ*ᵢ−θᵢ)² (RBD_helper_functions.jl:48-116). */
#define NJMAX 8
typedef struct {
  int nj, nu;
  double R0[NJMAX][9], p[NJMAX][3], ax[NJMAX][3], m[NJMAX], mc[NJMAX][3], Io[NJMAX][9], g[3], dt;
  double tgt[NJMAX], qw[NJMAX], rw[NJMAX], qfw[NJMAX];
} chain_t;

static void ch_rod(const double* a, double c, double s, const double* w, double* o) {
  const double axw[3] = {a[1] * w[2] - a[2] * w[1], a[2] * w[0] - a[0] * w[2], a[0] * w[1] - a[1] * w[0]};
  const double k = (1.0 - c) * (a[0] * w[0] + a[1] * w[1] + a[2] * w[2]);
  for (int r = 0; r < 3; ++r) o[r] = c * w[r] + s * axw[r] + k * a[r];
}
static void ch_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
static void ch_to_child(const chain_t* C, int i, double c, double s, const double* w, double* o) {
  double y[3];
  for (int r = 0; r < 3; ++r) y[r] = C->R0[i][r] * w[0] + C->R0[i][3 + r] * w[1] + C->R0[i][6 + r] * w[2];
  ch_rod(C->ax[i], c, -s, y, o);
}
static void ch_to_parent(const chain_t* C, int i, double c, double s, const double* w, double* o) {
  double y[3];
  ch_rod(C->ax[i], c, s, w, y);
  for (int r = 0; r < 3; ++r) o[r] = C->R0[i][3 * r] * y[0] + C->R0[i][3 * r + 1] * y[1] + C->R0[i][3 * r + 2] * y[2];
}
/* τ = M(q)q̈ + [qd] C(q,q̇)q̇ + [grav] g(q); qd may be NULL (zero velocity) */
static void ch_rnea(const chain_t* C, const double* cq, const double* sq, const double* qd,
                    const double* qdd, int grav, double* tau) {
  const int n = C->nj;
  double w[3] = {0, 0, 0}, v[3] = {0, 0, 0}, al[3] = {0, 0, 0}, ac[3];
  for (int r = 0; r < 3; ++r) ac[r] = grav ? -C->g[r] : 0.0;
  double fn[NJMAX][3], ff[NJMAX][3];
  for (int i = 0; i < n; ++i) {
    double t[3], u3[3], wi[3], vi[3], ali[3], aci[3];
    ch_to_child(C, i, cq[i], sq[i], w, wi);
    ch_cross(C->p[i], w, t);
    for (int r = 0; r < 3; ++r) u3[r] = v[r] - t[r];
    ch_to_child(C, i, cq[i], sq[i], u3, vi);
    ch_to_child(C, i, cq[i], sq[i], al, ali);
    ch_cross(C->p[i], al, t);
    for (int r = 0; r < 3; ++r) u3[r] = ac[r] - t[r];
    ch_to_child(C, i, cq[i], sq[i], u3, aci);
    if (qd) {
      double sqd[3];
      for (int r = 0; r < 3; ++r) sqd[r] = C->ax[i][r] * qd[i];
      for (int r = 0; r < 3; ++r) wi[r] += sqd[r];
      ch_cross(wi, sqd, t);
      for (int r = 0; r < 3; ++r) ali[r] += t[r];
      ch_cross(vi, sqd, t);
      for (int r = 0; r < 3; ++r) aci[r] += t[r];
    }
    for (int r = 0; r < 3; ++r) ali[r] += C->ax[i][r] * qdd[i];
    for (int r = 0; r < 3; ++r)
      fn[i][r] = C->Io[i][3 * r] * ali[0] + C->Io[i][3 * r + 1] * ali[1] + C->Io[i][3 * r + 2] * ali[2];
    ch_cross(C->mc[i], aci, t);
    for (int r = 0; r < 3; ++r) fn[i][r] += t[r];
    ch_cross(C->mc[i], ali, t);
    for (int r = 0; r < 3; ++r) ff[i][r] = C->m[i] * aci[r] - t[r];
    if (qd) {
      double hn[3], hf[3];
      for (int r = 0; r < 3; ++r)
        hn[r] = C->Io[i][3 * r] * wi[0] + C->Io[i][3 * r + 1] * wi[1] + C->Io[i][3 * r + 2] * wi[2];
      ch_cross(C->mc[i], vi, t);
      for (int r = 0; r < 3; ++r) hn[r] += t[r];
      ch_cross(C->mc[i], wi, t);
      for (int r = 0; r < 3; ++r) hf[r] = C->m[i] * vi[r] - t[r];
      ch_cross(wi, hn, t);
      for (int r = 0; r < 3; ++r) fn[i][r] += t[r];
      ch_cross(vi, hf, t);
      for (int r = 0; r < 3; ++r) fn[i][r] += t[r];
      ch_cross(wi, hf, t);
      for (int r = 0; r < 3; ++r) ff[i][r] += t[r];
    }
    memcpy(w, wi, sizeof w);
    memcpy(v, vi, sizeof v);
    memcpy(al, ali, sizeof al);
    memcpy(ac, aci, sizeof ac);
  }
  for (int i = n - 1; i >= 0; --i) {
    tau[i] = C->ax[i][0] * fn[i][0] + C->ax[i][1] * fn[i][1] + C->ax[i][2] * fn[i][2];
    if (i > 0) {
      double pf[3], pn[3], t[3];
      ch_to_parent(C, i, cq[i], sq[i], ff[i], pf);
      ch_to_parent(C, i, cq[i], sq[i], fn[i], pn);
      ch_cross(C->p[i], pf, t);
      for (int r = 0; r < 3; ++r) {
        fn[i - 1][r] += pn[r] + t[r];
        ff[i - 1][r] += pf[r];
      }
    }
  }
}
/* [q̇; v̇], v̇ = M \ (τ − bias) (RBD_helper_functions.jl:61-66) */
static void ch_xdot(const chain_t* C, const double* x, const double* u, double* xd) {
  const int n = C->nj;
  double cq[NJMAX], sq[NJMAX], zero[NJMAX], b[NJMAX], M[NJMAX][NJMAX], r[NJMAX], qdd[NJMAX];
  for (int i = 0; i < n; ++i) {
    cq[i] = cos(x[i]);
    sq[i] = sin(x[i]);
    zero[i] = 0.0;
  }
  ch_rnea(C, cq, sq, x + n, zero, 1, b);
  for (int k = 0; k < n; ++k) {
    double e[NJMAX], col[NJMAX];
    for (int j = 0; j < n; ++j) e[j] = j == k ? 1.0 : 0.0;
    ch_rnea(C, cq, sq, NULL, e, 0, col);
    for (int i = 0; i < n; ++i) M[i][k] = col[i];
  }
  for (int i = 0; i < n; ++i) r[i] = (i < C->nu ? u[i] : 0.0) - b[i];
  for (int k = 0; k < n; ++k) { /* Gaussian elimination, no pivoting (M SPD) */
    const double inv = 1.0 / M[k][k];
    for (int i = k + 1; i < n; ++i) {
      const double l = M[i][k] * inv;
      for (int j = k + 1; j < n; ++j) M[i][j] -= l * M[k][j];
      r[i] -= l * r[k];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    double acc = r[i];
    for (int j = i + 1; j < n; ++j) acc -= M[i][j] * qdd[j];
    qdd[i] = acc / M[i][i];
  }
  for (int i = 0; i < n; ++i) {
    xd[i] = x[n + i];
    xd[n + i] = qdd[i];
  }
}
static void ch_rk4(const chain_t* C, const double* x, const double* u, double* xn) {
  const int nx = 2 * C->nj;
  double k1[2 * NJMAX], k2[2 * NJMAX], k3[2 * NJMAX], k4[2 * NJMAX], y[2 * NJMAX] = {0};
  ch_xdot(C, x, u, k1);
  for (int i = 0; i < nx; ++i) { k1[i] *= C->dt; y[i] = x[i] + 0.5 * k1[i]; }
  ch_xdot(C, y, u, k2);
  for (int i = 0; i < nx; ++i) { k2[i] *= C->dt; y[i] = x[i] + 0.5 * k2[i]; }
  ch_xdot(C, y, u, k3);
  for (int i = 0; i < nx; ++i) { k3[i] *= C->dt; y[i] = x[i] + k3[i]; }
  ch_xdot(C, y, u, k4);
  for (int i = 0; i < nx; ++i) {
    k4[i] *= C->dt;
    xn[i] = x[i] + (1.0 / 6.0) * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
  }
}
static void ch_dyn(const prob_t* P, const double* x, const double* u, double* xn) {
  ch_rk4((const chain_t*)P->ext, x, u, xn);
}
static void ch_lin(const prob_t* P, int t, const double* x, const double* u, double* A, double* B) {
  (void)t;
  const chain_t* C = (const chain_t*)P->ext;
  const int nx = P->n, nu = P->m, nd = nx + nu;
  const double cbe = 6.0554544523933395e-6; /* ε^⅓, fp64 */
  double z[2 * NJMAX + NJMAX], fp[2 * NJMAX], fm[2 * NJMAX];
  for (int i = 0; i < nx; ++i) z[i] = x[i];
  for (int i = 0; i < nu; ++i) z[nx + i] = u[i];
  for (int k = 0; k < nd; ++k) {
    const double h = cbe * fmax(1.0, fabs(z[k]));
    double zp[2 * NJMAX + NJMAX], zm[2 * NJMAX + NJMAX];
    memcpy(zp, z, sizeof(double) * nd);
    memcpy(zm, z, sizeof(double) * nd);
    zp[k] = z[k] + h;
    zm[k] = z[k] - h;
    ch_rk4(C, zp, zp + nx, fp);
    ch_rk4(C, zm, zm + nx, fm);
    const double inv = 1.0 / (zp[k] - zm[k]);
    for (int i = 0; i < nx; ++i) {
      const double dv = (fp[i] - fm[i]) * inv;
      if (k < nx) A[i * nx + k] = dv; else B[i * nu + (k - nx)] = dv;
    }
  }
}
static void ch_quad(const prob_t* P, int t, const double* x, const double* u, double* qv, double* r,
                    double* Q, double* Pm, double* R) {
  (void)t;
  const chain_t* C = (const chain_t*)P->ext;
  const int n = C->nj, nx = P->n, nu = P->m;
  memset(qv, 0, sizeof(double) * nx);
  memset(Q, 0, sizeof(double) * nx * nx);
  memset(Pm, 0, sizeof(double) * nu * nx);
  memset(R, 0, sizeof(double) * nu * nu);
  for (int i = 0; i < n; ++i) {
    qv[i] = -2.0 * C->qw[i] * (C->tgt[i] - x[i]);
    Q[i * nx + i] = 2.0 * C->qw[i];
  }
  for (int k = 0; k < nu; ++k) {
    r[k] = 2.0 * C->rw[k] * u[k];
    R[k * nu + k] = 2.0 * C->rw[k];
  }
}
static void ch_fquad(const prob_t* P, const double* x, double* s, double* S) {
  const chain_t* C = (const chain_t*)P->ext;
  const int n = C->nj, nx = P->n;
  memset(s, 0, sizeof(double) * nx);
  memset(S, 0, sizeof(double) * nx * nx);
  for (int i = 0; i < n; ++i) {
    s[i] = -2.0 * C->qfw[i] * (C->tgt[i] - x[i]);
    S[i * nx + i] = 2.0 * C->qfw[i];
  }
}
static double ch_cost(const prob_t* P, const double* x, const double* u) {
  const chain_t* C = (const chain_t*)P->ext;
  double acc = 0.0;
  for (int i = 0; i < C->nj; ++i) {
    const double e = C->tgt[i] - x[i];
    acc = acc + C->qw[i] * e * e;
  }
  for (int k = 0; k < P->m; ++k) acc = acc + C->rw[k] * u[k] * u[k];
  return acc;
}
static double ch_fcost(const prob_t* P, const double* x) {
  const chain_t* C = (const chain_t*)P->ext;
  double acc = 0.0;
  for (int i = 0; i < C->nj; ++i) {
    const double e = C->tgt[i] - x[i];
    acc = acc + C->qfw[i] * e * e;
  }
  return acc;
}
/* chain constants from the URDF-derived arrays (ilqr_amd.urdf.Chain): rotational
 * inertia about the body origin Io = Ic + m(|c|²I − ccᵀ), first moment mc = m·c */
static int ch_init(chain_t* C, int nj, int nu, const double* R0, const double* p, const double* ax,
                   const double* mass, const double* com, const double* Ic, const double* grav,
                   double dt, const double* tgt, const double* qw, const double* rw,
                   const double* qfw) {
  if (nj < 1 || nj > NJMAX || nu < 1 || nu > nj || 2 * nj > NMAX) return -1;
  memset(C, 0, sizeof *C);
  C->nj = nj;
  C->nu = nu;
  C->dt = dt;
  for (int r = 0; r < 3; ++r) C->g[r] = grav[r];
  for (int i = 0; i < nj; ++i) {
    const double* c = com + 3 * i;
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    for (int k = 0; k < 9; ++k) C->R0[i][k] = R0[9 * i + k];
    for (int r = 0; r < 3; ++r) {
      C->p[i][r] = p[3 * i + r];
      C->ax[i][r] = ax[3 * i + r];
      C->mc[i][r] = mass[i] * c[r];
    }
    C->m[i] = mass[i];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        C->Io[i][3 * r + k] = Ic[9 * i + 3 * r + k] + mass[i] * ((r == k ? cc : 0.0) - c[r] * c[k]);
    C->tgt[i] = tgt[i];
    C->qw[i] = qw[i];
    C->qfw[i] = qfw[i];
  }
  for (int k = 0; k < nu; ++k) C->rw[k] = rw[k];
  return 0;
}

static prob_t instance(int b, int n, int m, int T, const double* A, const double* Bm,
                       const double* Q, const double* R, const double* Qf) {
  prob_t P = {n, m, T, A + (size_t)b * n * n, Bm + (size_t)b * n * m, Q + (size_t)b * n * n,
              R + (size_t)b * m * m, Qf + (size_t)b * n * n, NULL,
              lq_lin, lq_quad, lq_fquad, lq_dyn, lq_cost, lq_fcost};
  return P;
}

static void set_threads(int nthreads) {
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#else
  (void)nthreads;
#endif
}

int oracle_max_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

/* returns the number of trajectories with NaN gains; status may be NULL */
int oracle_lq_backward(int Bn, int T, int n, int m, const double* A, const double* Bm,
                       const double* Q, const double* R, const double* Qf, const double* x,
                       const double* u, double mu, int sym, double* d, double* K, int* status,
                       int nthreads) {
  if (n > NMAX || m > MMAX) return -1;
  set_threads(nthreads);
  int nans = 0;
#pragma omp parallel for schedule(static) reduction(+ : nans)
  for (int b = 0; b < Bn; ++b) {
    const prob_t P = instance(b, n, m, T, A, Bm, Q, R, Qf);
    const int bad = backward_one(&P, x + (size_t)b * (T + 1) * n, u + (size_t)b * T * m, mu, sym,
                                 d + (size_t)b * T * m, K + (size_t)b * T * m * n);
    if (status) status[b] = bad ? 4 : 0;
    nans += bad;
  }
  return nans;
}

int oracle_lq_forward(int Bn, int T, int n, int m, const double* A, const double* Bm,
                      const double* Q, const double* R, const double* Qf, const double* x,
                      const double* u, const double* xtraj, const double* d, const double* K,
                      const double* prev_cost, double* xnew, double* unew, double* cost,
                      int* trials, int max_trials, double alpha0, double shrink, int nthreads) {
  if (n > NMAX || m > MMAX) return -1;
  set_threads(nthreads);
  int fails = 0;
#pragma omp parallel for schedule(static) reduction(+ : fails)
  for (int b = 0; b < Bn; ++b) {
    const prob_t P = instance(b, n, m, T, A, Bm, Q, R, Qf);
    const int tr = forward_one(&P, x + (size_t)b * (T + 1) * n, u + (size_t)b * T * m,
                               xtraj ? xtraj + (size_t)b * (T + 1) * n : NULL,
                               d + (size_t)b * T * m, K + (size_t)b * T * m * n, prev_cost[b],
                               xnew + (size_t)b * (T + 1) * n, unew + (size_t)b * T * m, &cost[b],
                               max_trials, alpha0, shrink, NULL);
    if (trials) trials[b] = tr;
    fails += tr < 0;
  }
  return fails;
}

/* fit (forward_pass.jl:148-179) for one trajectory.
 * status: 1 converged, 2 max_iter, 3 LS exhausted, 4 NaN.
 * hcost / htrials / hdu2 (may be NULL): per iteration i (index i − 1) the accepted cost
 * (the reference's `Iteration: i  Total Cost: c` line, :167; NaN if the search failed),
 * the trials of the search (max_trials when exhausted), Σ(ū − u)² (:171); entries past
 * the last iteration untouched — ilqr_fit_ex's history record (include/ilqr.h). */
/* test-only (tests/test_reference_gifs.py::test_gif_pin_sensitivity): 1 = on convergence
 * return the iterate just computed instead of the reference's previous one (:171-178). */
static int FIT_RETURN_POST_UPDATE = 0;
void oracle_set_fit_return_post_update(int on) { FIT_RETURN_POST_UPDATE = on; }

static void fit_one(const prob_t* P, const double* x_init, const double* u_init,
                    const double* xtraj, int max_iter, double tol, double mu, int sym,
                    int max_trials, double alpha0, double shrink, double* x_out, double* u_out,
                    double* cost, int* iters, int* status, double* hcost, int* htrials,
                    double* hdu2, double* hgap) {
  const int n = P->n, m = P->m, T = P->T;
  const size_t xs = (size_t)(T + 1) * n, us = (size_t)T * m;
  double* buf = (double*)malloc(sizeof(double) * (2 * xs + 2 * us + us + us * n));
  double *xi = buf, *ui = xi + xs, *xn = ui + us, *un = xn + xs, *d = un + us, *K = d + us;
  memcpy(xi, x_init, sizeof(double) * xs);
  memcpy(ui, u_init, sizeof(double) * us);
  double prev_cost = INFINITY; /* :159 */
  int st = 2, it;
  for (it = 1; it <= max_iter; ++it) { /* :161 */
    if (backward_one(P, xi, ui, mu, sym, d, K)) { st = 4; break; }
    double nc = NAN, gap = INFINITY;
    const int tr = forward_one(P, xi, ui, xtraj, d, K, prev_cost, xn, un, &nc, max_trials, alpha0, shrink,
                               &gap);
    if (hgap) hgap[it - 1] = gap;
    if (htrials) htrials[it - 1] = tr < 0 ? max_trials : tr;
    if (hcost) hcost[it - 1] = tr < 0 ? NAN : nc;
    if (tr < 0) { st = (nc != nc) ? 4 : 3; break; }
    prev_cost = nc; /* :168 */
    double du2 = 0.0;
    for (size_t i = 0; i < us; ++i) du2 += (un[i] - ui[i]) * (un[i] - ui[i]);
    if (hdu2) hdu2[it - 1] = du2;
    if (du2 <= tol) { /* :171 — break before the update */
      st = 1;
      if (FIT_RETURN_POST_UPDATE) {
        memcpy(xi, xn, sizeof(double) * xs);
        memcpy(ui, un, sizeof(double) * us);
      }
      break;
    }
    memcpy(xi, xn, sizeof(double) * xs); /* :174-175 */
    memcpy(ui, un, sizeof(double) * us);
  }
  memcpy(x_out, xi, sizeof(double) * xs);
  memcpy(u_out, ui, sizeof(double) * us);
  *cost = prev_cost;
  if (iters) *iters = it > max_iter ? max_iter : it;
  if (status) *status = st;
  free(buf);
}

/* The fits and the chain iteration at the caller's alpha0 and shrink are the *_opt entries; the
 * entries of the earlier names keep their argument lists and run them at the defaults (1, 0.5).
 * History arrays (may be NULL) as oracle_tl_fit's; hgap: forward_one's gap of every iteration. */
int oracle_lq_fit_opt(int Bn, int T, int n, int m, const double* A, const double* Bm, const double* Q,
                  const double* R, const double* Qf, const double* x_init, const double* u_init,
                  const double* xtraj, int max_iter, double tol, double mu, int sym, int max_trials,
                  double alpha0, double shrink, double* x_out, double* u_out, double* cost,
                  int* iters, int* status, int nthreads, double* hcost, int* htrials,
                  double* hdu2, double* hgap) {
  if (n > NMAX || m > MMAX) return -1;
  set_threads(nthreads);
  const size_t xs = (size_t)(T + 1) * n, us = (size_t)T * m, hs = (size_t)max_iter;
#pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < Bn; ++b) {
    const prob_t P = instance(b, n, m, T, A, Bm, Q, R, Qf);
    fit_one(&P, x_init + b * xs, u_init + b * us, xtraj ? xtraj + b * xs : NULL, max_iter, tol, mu,
            sym, max_trials, alpha0, shrink, x_out + b * xs, u_out + b * us, &cost[b],
            iters ? &iters[b] : NULL,
            status ? &status[b] : NULL, hcost ? hcost + b * hs : NULL, htrials ? htrials + b * hs : NULL,
            hdu2 ? hdu2 + b * hs : NULL, hgap ? hgap + b * hs : NULL);
  }
  return 0;
}

int oracle_lq_fit(int Bn, int T, int n, int m, const double* A, const double* Bm, const double* Q,
                  const double* R, const double* Qf, const double* x_init, const double* u_init,
                  const double* xtraj, int max_iter, double tol, double mu, int sym, int max_trials,
                  double* x_out, double* u_out, double* cost, int* iters, int* status,
                  int nthreads) {
  return oracle_lq_fit_opt(Bn, T, n, m, A, Bm, Q, R, Qf, x_init, u_init, xtraj, max_iter, tol, mu, sym,
                           max_trials, 1.0, 0.5, x_out, u_out, cost, iters, status, nthreads, NULL, NULL,
                           NULL, NULL);
}

/* -- 2-link arm entry points (same conventions as the LQ ones) -- */
int oracle_tl_backward(int Bn, int T, int nu, const double* x, const double* u, double mu, int sym,
                       double* d, double* K, int* status, int nthreads) {
  set_threads(nthreads);
  const prob_t P = tl_problem(T, nu);
  int nans = 0;
#pragma omp parallel for schedule(static) reduction(+ : nans)
  for (int b = 0; b < Bn; ++b) {
    const int bad = backward_one(&P, x + (size_t)b * (T + 1) * 4, u + (size_t)b * T * nu, mu, sym,
                                 d + (size_t)b * T * nu, K + (size_t)b * T * nu * 4);
    if (status) status[b] = bad ? 4 : 0;
    nans += bad;
  }
  return nans;
}

int oracle_tl_forward(int Bn, int T, int nu, const double* x, const double* u, const double* xtraj,
                      const double* d, const double* K, const double* prev_cost, double* xnew,
                      double* unew, double* cost, int* trials, int max_trials, double alpha0,
                      double shrink, int nthreads) {
  set_threads(nthreads);
  const prob_t P = tl_problem(T, nu);
  int fails = 0;
#pragma omp parallel for schedule(static) reduction(+ : fails)
  for (int b = 0; b < Bn; ++b) {
    const int tr = forward_one(&P, x + (size_t)b * (T + 1) * 4, u + (size_t)b * T * nu,
                               xtraj ? xtraj + (size_t)b * (T + 1) * 4 : NULL, d + (size_t)b * T * nu,
                               K + (size_t)b * T * nu * 4, prev_cost[b], xnew + (size_t)b * (T + 1) * 4,
                               unew + (size_t)b * T * nu, &cost[b], max_trials, alpha0, shrink, NULL);
    if (trials) trials[b] = tr;
    fails += tr < 0;
  }
  return fails;
}

/* history arrays (may be NULL): (Bn, max_iter), trajectory slowest (see fit_one) */
int oracle_tl_fit_opt(int Bn, int T, int nu, const double* x_init, const double* u_init, const double* xtraj,
                  int max_iter, double tol, double mu, int sym, int max_trials, double alpha0,
                  double shrink, double* x_out, double* u_out, double* cost, int* iters, int* status,
                  int nthreads, double* hcost, int* htrials, double* hdu2) {
  set_threads(nthreads);
  const prob_t P = tl_problem(T, nu);
  const size_t xs = (size_t)(T + 1) * 4, us = (size_t)T * nu, hs = (size_t)max_iter;
#pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < Bn; ++b)
    fit_one(&P, x_init + b * xs, u_init + b * us, xtraj ? xtraj + b * xs : NULL, max_iter, tol, mu,
            sym, max_trials, alpha0, shrink, x_out + b * xs, u_out + b * us, &cost[b],
            iters ? &iters[b] : NULL,
            status ? &status[b] : NULL, hcost ? hcost + b * hs : NULL, htrials ? htrials + b * hs : NULL,
            hdu2 ? hdu2 + b * hs : NULL, NULL);
  return 0;
}

int oracle_tl_fit(int Bn, int T, int nu, const double* x_init, const double* u_init, const double* xtraj,
                  int max_iter, double tol, double mu, int sym, int max_trials, double* x_out,
                  double* u_out, double* cost, int* iters, int* status, int nthreads, double* hcost,
                  int* htrials, double* hdu2) {
  return oracle_tl_fit_opt(Bn, T, nu, x_init, u_init, xtraj, max_iter, tol, mu, sym, max_trials, 1.0, 0.5,
                           x_out, u_out, cost, iters, status, nthreads, hcost, htrials, hdu2);
}

/* backward_pass on caller-supplied tiles (ilqr_backward_tiles' checker). x/u are
 * only used for their shapes; the tiles carry everything. */
int oracle_tiles_backward(int Bn, int T, int n, int m, const double* A, const double* Bm,
                          const double* lx, const double* lu, const double* lxx, const double* lux,
                          const double* luu, const double* lfx, const double* lfxx, double mu,
                          int sym, double* d, double* K, int* status, int nthreads) {
  if (n > NMAX || m > MMAX) return -1;
  set_threads(nthreads);
  int nans = 0;
  double* dummy = (double*)calloc((size_t)(T + 1) * (n > m ? n : m), sizeof(double));
#pragma omp parallel for schedule(static) reduction(+ : nans)
  for (int b = 0; b < Bn; ++b) {
    const size_t bt = (size_t)b * T;
    const double* tl[9] = {A + bt * n * n, Bm + bt * n * m, lx + bt * n, lu + bt * m,
                           lxx + bt * n * n, lux ? lux + bt * m * n : NULL, luu + bt * m * m,
                           lfx + (size_t)b * n, lfxx + (size_t)b * n * n};
    prob_t P = {n, m, T, NULL, NULL, NULL, NULL, NULL, tl, tiles_lin, tiles_quad, tiles_fquad,
                NULL, NULL, NULL};
    const int bad = backward_one(&P, dummy, dummy, mu, sym, d + bt * m, K + bt * m * n);
    if (status) status[b] = bad ? 4 : 0;
    nans += bad;
  }
  free(dummy);
  return nans;
}

/* -- chain family exports (config 5 checker and CPU baseline) ------------------------ */
#define CH_ARGS                                                                                 \
  int nj, int nu, const double *R0, const double *p, const double *ax, const double *mass,      \
      const double *com, const double *Ic, const double *grav, double dt, const double *tgt,    \
      const double *qw, const double *rw, const double *qfw
#define CH_PASS nj, nu, R0, p, ax, mass, com, Ic, grav, dt, tgt, qw, rw, qfw

/* one RK4 step for n points: x (n, 2nj), u (n, nu) → xn (n, 2nj) */
int oracle_chain_dynamics(int npts, CH_ARGS, const double* x, const double* u, double* xn) {
  chain_t C;
  if (ch_init(&C, CH_PASS) != 0) return -1;
  for (int i = 0; i < npts; ++i) ch_rk4(&C, x + (size_t)i * 2 * nj, u + (size_t)i * nu, xn + (size_t)i * 2 * nj);
  return 0;
}

/* one cold-start fit iteration per trajectory (prev_cost = +Inf): backward_pass on the
 * central-difference linearisation, then forward_pass with the line search. */
int oracle_chain_iterate_opt(int Bn, int T, CH_ARGS, const double* x, const double* u, double mu,
                         int sym, int max_trials, double alpha0, double shrink, double* d, double* K,
                         double* xn, double* un, double* cost, int* trials, int nthreads) {
  chain_t C;
  if (ch_init(&C, CH_PASS) != 0) return -1;
  set_threads(nthreads);
  const int n = 2 * nj, m = nu;
  const size_t xs = (size_t)(T + 1) * n, us = (size_t)T * m;
  int nans = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : nans)
  for (int b = 0; b < Bn; ++b) {
    prob_t P = {n, m, T, NULL, NULL, NULL, NULL, NULL, NULL, ch_lin, ch_quad, ch_fquad,
                ch_dyn, ch_cost, ch_fcost, &C};
    const int bad = backward_one(&P, x + b * xs, u + b * us, mu, sym, d + b * us, K + b * us * n);
    nans += bad;
    const int tr = forward_one(&P, x + b * xs, u + b * us, NULL, d + b * us, K + b * us * n, INFINITY,
                               xn + b * xs, un + b * us, &cost[b], max_trials, alpha0, shrink, NULL);
    if (trials) trials[b] = tr;
  }
  return nans;
}

int oracle_chain_iterate(int Bn, int T, CH_ARGS, const double* x, const double* u, double mu,
                         int sym, int max_trials, double* d, double* K, double* xn, double* un,
                         double* cost, int* trials, int nthreads) {
  return oracle_chain_iterate_opt(Bn, T, CH_PASS, x, u, mu, sym, max_trials, 1.0, 0.5, d, K, xn, un, cost,
                                  trials, nthreads);
}
