// Host side shared by the chain objects (ilqr_chain.hip, ilqr_chain_tiles.hip): the handle
// behind include/ilqr.h's ilqr_chain_*, the chain constants in a kernel's value type, and the
// tiles path's interface — one table of entry points per joint count, defined by the object
// compiled for it (ilqr_chain_tiles.hip with -DILQR_CHAIN_NJ=4..7).
#pragma once
#include "ilqr_chain_model.h"
#include "ilqr_fit.h"
#include "ilqr_internal.h"

struct ilqr_chain_handle {
  int device = 0;
  int nj = 0, nu = 0, T = 0, batch = 0;
  int dtype = ILQR_F64;
  int lin = ILQR_LINEARIZE_DUAL;
  ilqr_chain chain{};
  hipStream_t stream = nullptr;
  // every device buffer, pinned word and event below is acquired through `own`: in
  // ilqr_chain_create, or at its first use (two.task_dev, tiles.joint_rows, tiles.task_rows,
  // tiles.path, tiles.path_goal)
  ilqr::HipOwned own;
  void* xbuf[2] = {nullptr, nullptr};
  void* ubuf[2] = {nullptr, nullptr};
  void* K = nullptr;
  void* d = nullptr;
  ilqr::FitState fit;  // the fit driver's per-trajectory state, words and events (ilqr_fit.h)
  // cost_functions.jl's factories (ilqr_chain_set_simple_costs, _set_task_costs): the mode and
  // the chain's joint-space weights as created (restored by ILQR_CHAIN_COST_JOINT)
  int32_t cost_mode = ILQR_CHAIN_COST_JOINT;
  ilqr_chain created{};
  bool task_mode() const { return cost_mode != ILQR_CHAIN_COST_JOINT; }

  // what 2-joint chains alone read (ilqr_chain.hip)
  struct TwoJoint {
    void* J = nullptr;  // the linearisation records
    // closed-form dynamics (ilqr_chain_set_dynamics): available once sampled and checked
    // against the recursion at creation, used unless RNEA is asked for
    bool trig_ok = false;
    int32_t dyn_mode = ILQR_CHAIN_DYN_AUTO;
    double trig_err = 0.0;  // the check's max relative error
    ilqr::ChainTrig<double> trig{};
    bool use_trig() const { return trig_ok && dyn_mode != ILQR_CHAIN_DYN_RNEA; }
    // the task-space final cost's coefficients in device memory
    ilqr::ChainTask* task_dev = nullptr;
    const ilqr::ChainTask* task(bool task_mode) const { return task_mode ? task_dev : nullptr; }
  } two;

  // what the tiles path alone reads (4..7 joints, fp64; ilqr_chain_tiles.hip)
  struct Tiles {
    // the derivative and cost tiles the tiles kernel reads and its per-trajectory status
    double *tA = nullptr, *tB = nullptr, *lx = nullptr, *lu = nullptr, *lxx = nullptr, *luu = nullptr;
    double *lfx = nullptr, *lfxx = nullptr;
    int32_t* bstatus = nullptr;
    // the task-space costs (ilqr_chain_set_task_costs): the kinematics are composed on the
    // device, these are the kernel argument
    ilqr::ChainTaskK taskk{};
    // a goal per trajectory (ilqr_chain_set_joint_targets, _set_task_targets): the handle's
    // copies of the rows, (batch, n_joints) and (batch, 3), allocated at the first call and
    // kept; `on` while an override is set. Each applies while its cost family is in effect.
    double *joint_rows = nullptr, *task_rows = nullptr;
    bool joint_rows_on = false, task_rows_on = false;
    // a tool path (ilqr_chain_set_task_path): the handle's copy of the (batch, T + 1, 3) rows,
    // a compact (batch, 3) copy of the rows T — trajectory b's final_target while the path is
    // set, handed to the kernels that read a goal row in place of task_rows — and the running
    // weight; allocated at the first call and kept. Applies while a task mode is in effect.
    double *path = nullptr, *path_goal = nullptr;
    double path_weight = 0.0;
    bool path_on = false;
    const double* goal_rows(bool task_mode) const {
      if (task_mode) return path_on ? path_goal : (task_rows_on ? task_rows : nullptr);
      return joint_rows_on ? joint_rows : nullptr;
    }
    const double* path_rows(bool task_mode) const { return task_mode && path_on ? path : nullptr; }
    // joint-velocity weights (ilqr_chain_set_velocity_weights): plain host values, handed to
    // the kernels by value while `vel_on`; they own no device memory and apply in every cost
    // mode, with or without goal rows and a path.
    double v_weight[ILQR_CHAIN_MAX_JOINTS] = {}, vf_weight[ILQR_CHAIN_MAX_JOINTS] = {};
    bool vel_on = false;
  } tiles;
};

namespace ilqr {

// The tiles path of one joint count (nu = NJ, nx = 2·NJ): the handle's operations in fp64
// under the names of ChainOps' (ilqr_chain.hip's dispatch hands either to the ABI functions),
// and f(x, u) alone in either dtype.
struct ChainTilesTable {
  using Value = double;
  // lxx, luu, lfxx of the cost in effect (at creation and at every change of the cost mode)
  hipError_t (*hessians)(ilqr_chain_handle* h);
  hipError_t (*linearize_to)(ilqr_chain_handle* h, const double* x, const double* u, double* A, double* Bm);
  hipError_t (*backward)(ilqr_chain_handle* h, const double* x, const double* u, double* d, double* K, int32_t* st,
                         double mu);
  hipError_t (*forward)(ilqr_chain_handle* h, const double* x, const double* u, const double* xt, const double* d,
                        const double* K, const double* pc, double* xn, double* un, double* nc, int32_t* tr,
                        int32_t* st, const LSParams& ls);
  hipError_t (*iteration)(ilqr_chain_handle* h, const ChainIter<double>& a, const LSParams& ls);
  // final_cost_quadratization at n states x[s·stride .. +nx)
  hipError_t (*quadratize)(ilqr_chain_handle* h, const double* x, size_t stride, int n, const int32_t* st,
                           double* cost, double* grad, double* hess);
  hipError_t (*dynamics)(ilqr_chain_handle* h, const double* x, const double* u, double* xo, int n);
  // an fp32 handle of this shape answers f(x, u) and nothing else
  hipError_t (*dynamics_f32)(ilqr_chain_handle* h, const float* x, const float* u, float* xo, int n);
};
extern const ChainTilesTable chain_tiles_table_4, chain_tiles_table_5, chain_tiles_table_6, chain_tiles_table_7;
const ChainTilesTable* chain_tiles_table(int nj);  // null outside 4..7 (ilqr_chain.hip)

}  // namespace ilqr

namespace {

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

// h->lin as a compile-time constant: fn(std::integral_constant<int, LIN>{}), for the kernels
// that carry both modes (ILQR_LINEARIZE_ANALYTIC is a kernel of its own, tiles path only:
// ChainTilesOps::linearize branches to it before coming here)
template <class Fn>
hipError_t with_lin(const ilqr_chain_handle* h, Fn&& fn) {
  if (h->lin == ILQR_LINEARIZE_DUAL) return fn(std::integral_constant<int, ILQR_LINEARIZE_DUAL>{});
  return fn(std::integral_constant<int, ILQR_LINEARIZE_CENTRAL_FD>{});
}

}  // namespace
