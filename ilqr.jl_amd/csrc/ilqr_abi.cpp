// C ABI of libilqr_hip.so (include/ilqr.h): handle/workspace management, argument
// validation with the reference's error behaviour mapped to status codes, and the
// fit driver (src/forward_pass.jl:148-179) on top of the fused iteration kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/ilqr.h"
#include "ilqr_fit.h"
#include "ilqr_internal.h"

constexpr int BW4_MIN_BATCH = 2048;  // default backward kernel switch (see bw_wave)

struct ilqr_handle {
  int device = 0;
  int nx = 0, nu = 0, T = 0, batch = 0;
  hipStream_t stream = nullptr;
  // everything below that lives on the device, in pinned memory or in the runtime is acquired
  // through `own` in ilqr_create and released with the handle; `pad_own` is the padded
  // scratch's group (ensure_pad)
  ilqr::HipOwned own, pad_own;
  // workspace (fit): ping-pong trajectories, gains, per-trajectory state
  double* xbuf[2] = {nullptr, nullptr};
  double* ubuf[2] = {nullptr, nullptr};
  double* K = nullptr;
  double* d = nullptr;
  ilqr::FitState fit;              // the fit driver's per-trajectory state, words and events (ilqr_fit.h)
  int32_t* host_status = nullptr;  // pinned host copy of a status array (fold_status)
  // LQ problems of another shape (nx ≤ 12, nu ≤ 4) run zero-padded on an inner
  // (12, 4) handle (created on the first such call): zero rows/columns of A, B, Q, R,
  // Qf, x, u decouple exactly, so the real entries are the (12, 4) kernels' bits.
  ilqr_handle* pad = nullptr;
  double *pA = nullptr, *pB = nullptr, *pQ = nullptr, *pR = nullptr, *pQf = nullptr;
  double *px = nullptr, *pu = nullptr, *pxt = nullptr, *pxn = nullptr, *pun = nullptr;
  double *pd = nullptr, *pK = nullptr;
  // 2-link arm: per-step linearisation workspace J = [A|B] (T × 24 × batch)
  double* J = nullptr;
  // pipelining: the batch is split into `nchunks` chunks; chunk i's forward pass
  // runs on `side` while chunk i+1's backward runs on `stream`
  hipStream_t side = nullptr;
  int nchunks = 1;
  // LQ family schedule (ilqr_set_schedule): fit through the pipelined kernel (forward
  // of half the workgroups overlapping the backward of the other half), and the
  // forward of sequential iterations through the LDS-ring kernel
  bool pipelined = false;
  bool fw_ring = true;
  bool fw_mfma = false;  // ILQR_SCHED_FORWARD_MFMA: the ring forward on the 4-block f64 MFMA
  // backward + forward of an iteration in one launch (ILQR_SCHED_FUSED, default on),
  // with the four-trajectories-per-wave backward and the ring forward only: 166 → 159 µs
  // per headline iteration (no kernel boundary)
  bool fused = true;
  // backward kernel of the LQ family: ILQR_SCHED_BACKWARD_WAVE (or PIPELINED) forces
  // one trajectory per wave, ILQR_SCHED_BACKWARD_BLOCK four per wave; by default four
  // per wave from BW4_MIN_BATCH trajectories up (below it there are fewer waves than
  // SIMDs and the shorter per-wave chain of the one-trajectory kernel wins:
  // profiles/r01/bw4_scan.txt)
  bool bw_wave = false;
  // the fused LQ iteration's cooperative line search (ILQR_SCHED_SEQUENTIAL_SEARCH
  // turns it off): per-trajectory records, candidate costs, the publication list and
  // its counters (zeroed here, re-armed by every launch's last wave)
  bool coop = true;
  // gain reuse on the fused path: within one fit call the gains K and the backward's
  // solve operands are the same in every iteration (A, B, Q, R, Qf, μ fixed), so the
  // first iteration stores the factor of H + μI here and the later ones run the
  // vector-only backward on it. ILQR_SCHED_FULL_BACKWARD turns it off; nullptr (not (12, 4), or
  // the allocation failed): every iteration runs the full recursion
  bool full_bw = false;
  double* fac = nullptr;
  // ... and across fit calls: K and fac stay valid for the next fit as long as the operands
  // they were computed from (IterArgs::snap, the storing wave's snapshot) and μ are the
  // same bits. The next fit's first iteration checks that on the device, wave by wave
  // (lq_iter_fused4_check_kernel), and re-factors only where it fails.
  // ILQR_SCHED_REUSE_PER_CALL turns it off; snap == nullptr (the allocation failed): off.
  bool per_call = false;
  double* snap = nullptr;
  int32_t* branch = nullptr;  // per wave of the last fit's first iteration: 1 reused, 0 re-factored
  bool branch_set = false;    // the last fit wrote `branch` (ilqr_reuse_record)
  // K, fac and snap are those of a fit on the fused reuse path that returned without a HIP
  // error, at μ = reuse_mu; cleared on entry of everything else that writes K or fac
  bool reuse_valid = false;
  double reuse_mu = 0.0;
  bool check_now = false;  // ilqr_fit_ex → enqueue_iteration: this fit's first launch checks
  // ILQR_TRACK_CONSISTENT (ilqr_set_tracking): the backward of ilqr_iterate / ilqr_fit takes
  // lx_t from x_t − x_traj_t (IterArgs::track). x_traj is vector-side data: the stored gains,
  // the factor and the snapshot do not depend on it, so neither the mode nor a new reference
  // touches reuse_valid
  bool track = false;
  ilqr::LSCoopRec* coop_rec = nullptr;
  double* coop_cost = nullptr;
  double* coop_du2 = nullptr;
  uint64_t* coop_list = nullptr;
  int32_t* coop_ctl = nullptr;
  uint32_t coop_gen = 0;  // fused launches so far (the list's generation tag)
  double* coop_sx = nullptr;  // the search's scratch rollouts (LSCoop::sx / su)
  double* coop_su = nullptr;
  ilqr::LSCoop* coop_dev = nullptr;  // the struct of the above, in device memory
  int bound[3] = {0, 0, 0};
  hipEvent_t ev_bw[2] = {nullptr, nullptr};
  hipEvent_t ev_fw[2] = {nullptr, nullptr};
};

namespace ilqr {

LSParams ls_params(const ilqr_options* o) {
  ilqr_options def;
  ilqr_default_options(&def);
  if (!o) o = &def;
  return LSParams{o->mu, o->alpha0, o->shrink, o->tol, o->max_trials};
}

ilqr_status check_options(const ilqr_options* o) {
  if (!o) return ILQR_OK;
  if (o->max_trials < 1 || o->max_iter < 0) return ILQR_ERR_BAD_ARG;
  if (!(o->shrink > 0.0 && o->shrink < 1.0) || !(o->alpha0 > 0.0) || std::isnan(o->mu))
    return ILQR_ERR_BAD_ARG;
  return ILQR_OK;
}

hipError_t fold_status(const int32_t* dev_status, int n, hipStream_t s, int32_t* host, ilqr_status* out) {
  std::vector<int32_t> tmp(host ? 0 : n);
  int32_t* st = host ? host : tmp.data();  // a pinned `host`: one DMA, no staging copy
  hipError_t e = hipMemcpyAsync(st, dev_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  bool nan = false, ls = false;
  for (int b = 0; b < n; ++b) {
    nan |= st[b] == ILQR_TRAJ_NAN;
    ls |= st[b] == ILQR_TRAJ_LS_EXHAUSTED;
  }
  *out = nan ? ILQR_ERR_NAN : (ls ? ILQR_ERR_LS_EXHAUSTED : ILQR_OK);
  return hipSuccess;
}

}  // namespace ilqr

namespace {

thread_local std::string g_last_error;

#define HIP_TRY(expr) ILQR_HIP_TRY(g_last_error, expr)

ilqr::LQParams lq_params(const ilqr_problem* p) {
  return ilqr::LQParams{p->A, p->B, p->Q, p->R, p->Qf};
}

constexpr int PAD_NX = 12, PAD_NU = 4;  // the compiled LQ shape padded problems run at

bool lq_paddable(int nx, int nu) {
  return !ilqr::lq_supported(nx, nu) && nx <= PAD_NX && nu <= PAD_NU &&
         ilqr::lq_supported(PAD_NX, PAD_NU);
}

ilqr_status check_problem(const ilqr_handle* h, const ilqr_problem* p) {
  if (!h || !p) return ILQR_ERR_BAD_ARG;
  if (p->kind == ILQR_PROBLEM_LQ) {
    if (!p->A || !p->B || !p->Q || !p->R || !p->Qf) return ILQR_ERR_BAD_ARG;
    if (!ilqr::lq_supported(h->nx, h->nu) && !lq_paddable(h->nx, h->nu)) return ILQR_ERR_UNSUPPORTED;
    return ILQR_OK;
  }
  if (p->kind == ILQR_PROBLEM_TWO_LINK) {
    // the arm is fully defined by the reference script: no per-instance data
    if (p->A || p->B || p->Q || p->R || p->Qf) return ILQR_ERR_BAD_ARG;
    if (!ilqr::tl_supported(h->nx, h->nu) || !h->J) return ILQR_ERR_UNSUPPORTED;
    return ILQR_OK;
  }
  return ILQR_ERR_UNSUPPORTED;
}

bool two_link(const ilqr_problem* p) { return p->kind == ILQR_PROBLEM_TWO_LINK; }

// the consistent tracking mode is the LQ family's (the 2-link family: a follow-up)
ilqr_status check_tracking(const ilqr_handle* h, const ilqr_problem* p) {
  return h->track && two_link(p) ? ILQR_ERR_UNSUPPORTED : ILQR_OK;
}

bool padded(const ilqr_handle* h, const ilqr_problem* p) {
  return p->kind == ILQR_PROBLEM_LQ && lq_paddable(h->nx, h->nu);
}

ilqr_status join(ilqr_handle* h, const ilqr_problem* p);

// the LQ iteration runs as one lq_iter_fused4 launch (enqueue_iteration)
bool fused_path(const ilqr_handle* h, const ilqr_problem* p) {
  return !two_link(p) && h->nchunks == 1 && h->fused && !h->bw_wave && h->fw_ring && h->nx == 12 &&
         h->nu == 4;
}

// Enqueue one fit iteration for the whole batch: backward(c) on the handle's
// stream, forward(c) on the side stream after it. With `chain`, backward(c) first
// waits for the previous iteration's forward(c) (same trajectories); otherwise the
// call ends by making the handle's stream wait for every forward (join).
ilqr_status enqueue_iteration(ilqr_handle* h, const ilqr_problem* p, const ilqr::IterArgs& a,
                              const ilqr::LSParams& ls, bool chain, const ilqr_history* hist = nullptr) {
  if (two_link(p)) {  // one stream: linearise, backward, forward
    HIP_TRY(ilqr::launch_tl_iteration(ilqr::two_link_params(), h->nu, h->batch, h->T, a, h->J, ls,
                                      h->stream));
    return ILQR_OK;
  }
  const ilqr::LQParams P = lq_params(p);
  if (h->nchunks == 1) {  // one stream, no cross-stream events (each hand-off costs ~10 µs)
    if (fused_path(h, p)) {
      ilqr::IterArgs ac = a;
      // only a launch that gets the list also re-arms it (ctl[(gen + 1) & 1] = 0): a
      // sequential-search launch between two cooperative ones must not advance the
      // generation, or the next cooperative launch would count in a half nobody zeroed
      // Against prev_cost = +Inf (a cold iteration, fit's first) trial 1 accepts every
      // finite cost (forward_pass.jl:77-80): nothing would be published, so the launch
      // runs the sequential search (the same bits) without the search's exit test.
      const bool coop = h->coop && a.prev_cost && !a.init;
      ac.coop = coop ? h->coop_dev : nullptr;
      ac.coop_ctl = coop ? h->coop_ctl : nullptr;
      ac.coop_gen = coop ? ++h->coop_gen : h->coop_gen;
      // fit's iterations ≥ 2 reuse the gains and the factor its first one stored
      const bool vec = a.fac && a.iter >= 2;
      // its first one checks the handle's stored gains against the problem instead, if
      // ilqr_fit_ex found them valid
      const bool check = !vec && a.init && a.fac && a.snap && h->check_now;
      HIP_TRY(ilqr::launch_lq_iter_fused4(P, h->batch, h->T, ac, ls, h->stream, h->fw_mfma, vec, check));
      return ILQR_OK;
    }
    HIP_TRY(ilqr::launch_lq_iter_backward(h->nx, h->nu, P, 0, h->batch, h->T, a, ls.mu, h->stream, h->bw_wave));
    HIP_TRY(ilqr::launch_lq_iter_forward(h->nx, h->nu, P, 0, h->batch, h->T, a, ls, h->stream, h->fw_ring,
                                         h->fw_mfma));
    return ILQR_OK;
  }
  for (int c = 0; c < h->nchunks; ++c) {
    const int b0 = h->bound[c], b1 = h->bound[c + 1];
    if (chain) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_fw[c], 0));
    HIP_TRY(ilqr::launch_lq_iter_backward(h->nx, h->nu, P, b0, b1, h->T, a, ls.mu, h->stream, h->bw_wave));
    HIP_TRY(hipEventRecord(h->ev_bw[c], h->stream));
    HIP_TRY(hipStreamWaitEvent(h->side, h->ev_bw[c], 0));
    HIP_TRY(ilqr::launch_lq_iter_forward(h->nx, h->nu, P, b0, b1, h->T, a, ls, h->side));
    if (hist)  // chunk c's record before ev_fw[c]: its next backward (it may set NAN) waits
               // for this chunk's record only, and still overlaps the next chunk's forward
      HIP_TRY(ilqr::launch_record_history(
          b1 - b0, a.iter, a.status + b0, a.iters + b0, a.trials + b0, a.new_cost + b0, a.du2 + b0, false,
          ls.alpha0, ls.shrink, hist->cost ? hist->cost + b0 : nullptr, hist->trials ? hist->trials + b0 : nullptr,
          hist->alpha ? hist->alpha + b0 : nullptr, hist->du2 ? hist->du2 + b0 : nullptr, h->side, h->batch));
    HIP_TRY(hipEventRecord(h->ev_fw[c], h->side));
  }
  if (!chain) return join(h, p);
  return ILQR_OK;
}

ilqr_status join(ilqr_handle* h, const ilqr_problem* p) {
  if (two_link(p) || h->nchunks == 1) return ILQR_OK;
  for (int c = 0; c < h->nchunks; ++c) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_fw[c], 0));
  return ILQR_OK;
}

// Inner (12, 4) handle and padded scratch, created on the first padded call (the
// only allocation outside ilqr_create); stream and schedule follow the outer handle.
// h->pad is published only once the whole group exists: a failure releases what was made,
// and the next padded call starts again from nothing.
ilqr_status ensure_pad(ilqr_handle* h) {
  if (!h->pad) {
    ilqr_handle* in = nullptr;
    const ilqr_status st = ilqr_create(&in, h->device, PAD_NX, PAD_NU, h->T, h->batch);
    if (st != ILQR_OK) return st;
    const size_t B = (size_t)h->batch, T = (size_t)h->T;
    ilqr::HipOwned& own = h->pad_own;
    own.dev(&h->pA, B * PAD_NX * PAD_NX);
    own.dev(&h->pB, B * PAD_NX * PAD_NU);
    own.dev(&h->pQ, B * PAD_NX * PAD_NX);
    own.dev(&h->pR, B * PAD_NU * PAD_NU);
    own.dev(&h->pQf, B * PAD_NX * PAD_NX);
    own.dev(&h->px, B * (T + 1) * PAD_NX);
    own.dev(&h->pxt, B * (T + 1) * PAD_NX);
    own.dev(&h->pxn, B * (T + 1) * PAD_NX);
    own.dev(&h->pu, B * T * PAD_NU);
    own.dev(&h->pun, B * T * PAD_NU);
    own.dev(&h->pd, B * T * PAD_NU);
    own.dev(&h->pK, B * T * PAD_NU * PAD_NX);
    if (!own.ok()) {
      const hipError_t e = own.error();
      own.release();
      (void)ilqr_destroy(in);
      return ilqr::hip_fail(g_last_error, e, "ilqr: padded workspace");
    }
    h->pad = in;
  }
  h->pad->stream = h->stream;
  h->pad->pipelined = h->pipelined;
  h->pad->fused = h->fused;
  h->pad->fw_ring = h->fw_ring;
  h->pad->fw_mfma = h->fw_mfma;
  h->pad->bw_wave = h->bw_wave;
  h->pad->coop = h->coop;
  h->pad->full_bw = h->full_bw;
  h->pad->per_call = h->per_call;
  h->pad->track = h->track;
  return ILQR_OK;
}

// (N, R, C) → (N, R2, C2) zero-padded, and back
ilqr_status pad3(ilqr_handle* h, const double* src, double* dst, size_t N, int R, int C, int R2, int C2) {
  HIP_TRY(ilqr::launch_pad3(src, dst, N, R, C, R2, C2, h->stream));
  return ILQR_OK;
}
ilqr_status unpad3(ilqr_handle* h, const double* src, double* dst, size_t N, int R, int C, int R2, int C2) {
  HIP_TRY(ilqr::launch_unpad3(src, dst, N, R, C, R2, C2, h->stream));
  return ILQR_OK;
}

#define ILQR_TRY(expr)                    \
  do {                                    \
    const ilqr_status s_ = (expr);        \
    if (s_ != ILQR_OK) return s_;         \
  } while (0)

// pad the LQ problem data into the scratch and describe it
ilqr_status pad_problem(ilqr_handle* h, const ilqr_problem* p, ilqr_problem* pp) {
  const size_t B = (size_t)h->batch;
  const int n = h->nx, m = h->nu;
  ILQR_TRY(pad3(h, p->A, h->pA, B, n, n, PAD_NX, PAD_NX));
  ILQR_TRY(pad3(h, p->B, h->pB, B, n, m, PAD_NX, PAD_NU));
  ILQR_TRY(pad3(h, p->Q, h->pQ, B, n, n, PAD_NX, PAD_NX));
  ILQR_TRY(pad3(h, p->R, h->pR, B, m, m, PAD_NU, PAD_NU));
  ILQR_TRY(pad3(h, p->Qf, h->pQf, B, n, n, PAD_NX, PAD_NX));
  *pp = *p;
  pp->A = h->pA;
  pp->B = h->pB;
  pp->Q = h->pQ;
  pp->R = h->pR;
  pp->Qf = h->pQf;
  return ILQR_OK;
}
// trajectories: x-like (B, T+1, nx), u-like (B, T, nu), gains K (B·T, nu, nx)
ilqr_status pad_x(ilqr_handle* h, const double* x, double* px) {
  return pad3(h, x, px, (size_t)h->batch, h->T + 1, h->nx, h->T + 1, PAD_NX);
}
ilqr_status pad_u(ilqr_handle* h, const double* u, double* pu) {
  return pad3(h, u, pu, (size_t)h->batch, h->T, h->nu, h->T, PAD_NU);
}
ilqr_status unpad_x(ilqr_handle* h, const double* px, double* x) {
  return unpad3(h, px, x, (size_t)h->batch, h->T + 1, h->nx, h->T + 1, PAD_NX);
}
ilqr_status unpad_u(ilqr_handle* h, const double* pu, double* u) {
  return unpad3(h, pu, u, (size_t)h->batch, h->T, h->nu, h->T, PAD_NU);
}

}  // namespace

// The stream's last kernel of a fit (gather_flags_kernel) stores the fit's number into
// the host-mapped call-status word as it runs, after every earlier kernel of the stream
// completed (in-order stream): when the word carries the number, the outputs are written.
// The host waits on that word by ilqr_wait.h's policy (spin around the expected end, nap
// only through the bulk of a wait expected to exceed 1 ms, sized per iteration). A
// headline-size fit (≈450 µs) never naps; a long one (a config-5 default fit, 2-9 ms; the
// floating family's fits; every shard thread of ilqr_multi) holds no core. The fit
// drivers' per-iteration convergence polls wait the same way on their events (wait_event;
// the next iteration is already queued). hipEventSynchronize busy-waits on this ROCm
// whatever the event's flags (profiles/r05/event_wait_probe_r05.log), so no runtime sync
// is left on these paths. ILQR_FIT_WAIT=sync in the environment forces the stream sync (A/B).
hipError_t ilqr::wait_host_seq(const volatile int32_t* w, uint32_t seq, int units, hipStream_t s,
                               HostWait* hw) {
  static const bool spin = [] {
    const char* e = getenv("ILQR_FIT_WAIT");
    return !(e && strcmp(e, "sync") == 0);
  }();
  if (!spin) return hipStreamSynchronize(s);
  auto done = [&] { return ((uint32_t)__atomic_load_n(w, __ATOMIC_ACQUIRE) >> 2) == seq; };
  hipError_t e = nap_spin_wait(hw, units, hipSuccess, hipErrorNotReady, done, [&] {
    const hipError_t q = hipStreamQuery(s);  // idle, busy (NotReady) or an execution error
    return q == hipSuccess && !done() ? hipErrorLaunchFailure : q;  // idle without the word: lost
  });
  return e != hipSuccess ? e : hipPeekAtLastError();  // a launch error of this thread
}

hipError_t ilqr::wait_event(hipEvent_t ev, HostWait* hw) {
  hipError_t q = hipErrorNotReady;
  auto done = [&] { return (q = hipEventQuery(ev)) != hipErrorNotReady; };
  const hipError_t e = nap_spin_wait(hw, 1, hipSuccess, hipErrorNotReady, done, [&] { return q = hipEventQuery(ev); });
  return e != hipSuccess ? e : q;
}

extern "C" {

int ilqr_abi_version(void) { return ILQR_ABI_VERSION; }

const char* ilqr_status_string(ilqr_status s) {
  switch (s) {
    case ILQR_OK: return "ok";
    case ILQR_ERR_BAD_DIMS: return "bad dimensions (size(x,1) must equal size(u,1)+1)";
    case ILQR_ERR_BAD_ARG: return "bad argument";
    case ILQR_ERR_UNSUPPORTED: return "unsupported problem kind or (nx, nu)";
    case ILQR_ERR_HIP: return "HIP runtime error";
    case ILQR_ERR_NAN: return "NaN in a trajectory";
    case ILQR_ERR_LS_EXHAUSTED: return "line search exhausted";
  }
  return "unknown status";
}

const char* ilqr_last_error(void) { return g_last_error.c_str(); }

void ilqr_default_options(ilqr_options* o) {
  if (!o) return;
  o->max_iter = 100;     // forward_pass.jl:152
  o->max_trials = 64;    // reference is unbounded (forward_pass.jl:70); 0.5^63 ≈ 1e-19
  o->tol = 1e-6;         // forward_pass.jl:152
  o->mu = 0.01;          // backward_pass.jl:214
  o->alpha0 = 1.0;       // forward_pass.jl:66
  o->shrink = 0.5;       // forward_pass.jl:82
}

int ilqr_supported(int32_t kind, int nx, int nu) {
  if (kind == ILQR_PROBLEM_LQ) return (ilqr::lq_supported(nx, nu) || lq_paddable(nx, nu)) ? 1 : 0;
  if (kind == ILQR_PROBLEM_TWO_LINK) return ilqr::tl_supported(nx, nu) ? 1 : 0;
  if (kind == ILQR_PROBLEM_TILES) return ilqr::tiles_supported(nx, nu) ? 1 : 0;
  if (kind == ILQR_PROBLEM_CHAIN) return (nx % 2 == 0) ? ilqr_chain_supported(nx / 2, nu) : 0;
  return 0;
}

ilqr_status ilqr_create(ilqr_handle** out, int device, int nx, int nu, int T, int batch) {
  if (!out) return ILQR_ERR_BAD_ARG;
  *out = nullptr;
  if (nx <= 0 || nu <= 0 || T <= 0 || batch <= 0) return ILQR_ERR_BAD_DIMS;
  HIP_TRY(hipSetDevice(device));
  auto* h = new ilqr_handle;
  h->device = device;
  h->nx = nx;
  h->nu = nu;
  h->T = T;
  h->batch = batch;
  h->bw_wave = batch < BW4_MIN_BATCH;
  const size_t B = (size_t)batch;
  ilqr::HipOwned& own = h->own;
  own.set_device(device);
  h->pad_own.set_device(device);
  for (int i = 0; i < 2; ++i) {
    own.dev(&h->xbuf[i], B * (T + 1) * nx);
    own.dev(&h->ubuf[i], B * T * nu);
  }
  own.dev(&h->K, B * T * nu * nx);
  own.dev(&h->d, B * T * nu);
  hipError_t e = ilqr::fit_state_create(&h->fit, own, B, sizeof(double));
  own.pinned(&h->host_status, B, hipHostMallocDefault);
  int nsl = 0;  // the search's scratch slots
  if (nx == 12 && nu == 4) {
    own.dev(&h->coop_rec, B);
    own.dev(&h->coop_cost, B * ilqr::COOP_MAX_TRIALS);
    own.dev(&h->coop_du2, B * ilqr::COOP_MAX_TRIALS);
    own.dev_zero(&h->coop_list, B);  // generation 0: stale
    own.dev_zero(&h->coop_ctl, 2);
    own.dev(&h->coop_dev, 1);
    // scratch rollouts for the first searches of a launch (32-bit buffer offsets: the
    // x part must stay under 2 GiB, else no scratch)
    nsl = std::min(batch, ilqr::COOP_SCRATCH_SLOTS);
    const size_t sx = (size_t)nsl * ilqr::COOP_MAX_TRIALS * (size_t)(T + 1) * nx;
    const size_t su = (size_t)nsl * ilqr::COOP_MAX_TRIALS * (size_t)T * nu;
    // the scratch (≈260 MB at T = 1000) is a speed-up, not a need: without it the search
    // rolls the final trial out again (nslots = 0), so a failed allocation is not an error
    const bool fits = sizeof(double) * sx < (size_t(1) << 31);
    if (!(fits && own.try_dev(&h->coop_sx, sx) && own.try_dev(&h->coop_su, su))) {
      own.drop(&h->coop_sx);
      nsl = 0;
    }
    // the backward's factor of H + μI of one fit's first iteration (80 B per trajectory
    // and step, 33 MB at B = 4096, T = 100); like the scratch a speed-up, not a need.
    // The operand snapshot of those gains (31 doubles per lane: the size of the problem
    // itself, 16 MB at B = 4096) and the per-wave branch record; without them reuse stays
    // within one call
    if (own.try_dev(&h->fac, ilqr::lq_fac_doubles(B, T)) &&
        !(own.try_dev(&h->snap, ilqr::lq_snap_doubles(B)) && own.try_dev(&h->branch, ilqr::lq_fused_waves(B))))
      own.drop(&h->snap);
  }
  if (ilqr::tl_supported(nx, nu)) own.dev(&h->J, ilqr::tl_workspace_doubles(batch, T));
  own.stream(&h->side, hipStreamNonBlocking);
  for (int c = 0; c < 2; ++c) {
    own.event(&h->ev_bw[c], hipEventDisableTiming);
    own.event(&h->ev_fw[c], hipEventDisableTiming);
  }
  if (!own.ok()) e = own.error();
  if (e == hipSuccess && h->coop_dev) {  // the struct of the search's buffers, and the zeroing done
    const ilqr::LSCoop c{h->coop_rec, h->coop_cost, h->coop_du2, h->coop_list, h->coop_ctl,
                         h->coop_sx,  h->coop_su,   nsl};
    e = hipMemcpy(h->coop_dev, &c, sizeof(c), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) {
    // Two chunks (chunk c's forward on the side stream overlapping chunk c+1's
    // backward) only when each chunk still fills every SIMD with 4 backward waves:
    // measured at B = 4096 on MI355X, halves at 2 waves/SIMD run 14 % slower and
    // the cross-stream hand-offs cost ~10 µs each, a net loss.
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    const int full_gen = 4 * 4 * (cus > 0 ? cus : 256);
    h->nchunks = batch >= 2 * full_gen ? 2 : 1;
    h->bound[0] = 0;
    h->bound[h->nchunks] = batch;
    if (h->nchunks == 2) h->bound[1] = batch / 2;
  }
  if (e != hipSuccess) {
    ilqr_destroy(h);
    return ilqr::hip_fail(g_last_error, e, "ilqr_create: hipMalloc");
  }
  *out = h;
  return ILQR_OK;
}

ilqr_status ilqr_destroy(ilqr_handle* h) {
  if (!h) return ILQR_OK;
  (void)ilqr_destroy(h->pad);
  delete h;  // its owners release
  return ILQR_OK;
}

ilqr_status ilqr_set_stream(ilqr_handle* h, void* s) {
  if (!h) return ILQR_ERR_BAD_ARG;
  h->stream = (hipStream_t)s;
  return ILQR_OK;
}

ilqr_status ilqr_set_schedule(ilqr_handle* h, int flags) {
  if (!h || (flags & ~(ILQR_SCHED_PIPELINED | ILQR_SCHED_RING_FORWARD | ILQR_SCHED_BACKWARD_WAVE |
                      ILQR_SCHED_BACKWARD_BLOCK | ILQR_SCHED_FUSED | ILQR_SCHED_FORWARD_MFMA |
                      ILQR_SCHED_SEQUENTIAL_SEARCH | ILQR_SCHED_FULL_BACKWARD |
                      ILQR_SCHED_REUSE_PER_CALL)) != 0)
    return ILQR_ERR_BAD_ARG;
  // every combination check before any handle state changes
  if ((flags & ILQR_SCHED_FUSED) && (flags & (ILQR_SCHED_BACKWARD_WAVE | ILQR_SCHED_PIPELINED)))
    return ILQR_ERR_BAD_ARG;
  if ((flags & ILQR_SCHED_BACKWARD_BLOCK) && (flags & (ILQR_SCHED_BACKWARD_WAVE | ILQR_SCHED_PIPELINED)))
    return ILQR_ERR_BAD_ARG;
  for (ilqr_handle* t : {h, h->pad}) {
    if (!t) continue;
    t->pipelined = (flags & ILQR_SCHED_PIPELINED) != 0;
    t->fused = (flags & ILQR_SCHED_FUSED) != 0;
    t->fw_ring = (flags & ILQR_SCHED_RING_FORWARD) != 0;
    t->fw_mfma = (flags & ILQR_SCHED_FORWARD_MFMA) != 0;
    t->coop = (flags & ILQR_SCHED_SEQUENTIAL_SEARCH) == 0;
    t->full_bw = (flags & ILQR_SCHED_FULL_BACKWARD) != 0;
    t->per_call = (flags & ILQR_SCHED_REUSE_PER_CALL) != 0;
    t->bw_wave = (flags & (ILQR_SCHED_BACKWARD_WAVE | ILQR_SCHED_PIPELINED)) != 0 ||
                 (!(flags & ILQR_SCHED_BACKWARD_BLOCK) && h->batch < BW4_MIN_BATCH);
  }
  return ILQR_OK;
}

ilqr_status ilqr_set_tracking(ilqr_handle* h, int32_t mode) {
  if (!h || (mode != ILQR_TRACK_FORWARD_ONLY && mode != ILQR_TRACK_CONSISTENT)) return ILQR_ERR_BAD_ARG;
  for (ilqr_handle* t : {h, h->pad})
    if (t) t->track = mode == ILQR_TRACK_CONSISTENT;
  return ILQR_OK;
}

int32_t ilqr_get_tracking(const ilqr_handle* h) {
  return !h ? -1 : (h->track ? ILQR_TRACK_CONSISTENT : ILQR_TRACK_FORWARD_ONLY);
}

ilqr_status ilqr_sync(ilqr_handle* h) {
  if (!h) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ILQR_OK;
}

ilqr_status ilqr_backward(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                          const double* x, const double* u, double* d, double* K,
                          int32_t* status) {
  return ilqr_backward_tracking(h, p, o, x, u, nullptr, d, K, status);
}

// x_traj == nullptr: ilqr_backward itself (every family, the plain kernels)
ilqr_status ilqr_backward_tracking(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                                   const double* x, const double* u, const double* x_traj,
                                   double* d, double* K, int32_t* status) {
  ilqr_status st = check_problem(h, p);
  if (st != ILQR_OK) return st;
  if ((st = ilqr::check_options(o)) != ILQR_OK) return st;
  if (!x || !u || !d || !K) return ILQR_ERR_BAD_ARG;
  if (x_traj && two_link(p)) return ILQR_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(h->device));
  if (padded(h, p)) {
    ILQR_TRY(ensure_pad(h));
    ilqr_problem pp;
    ILQR_TRY(pad_problem(h, p, &pp));
    ILQR_TRY(pad_x(h, x, h->px));
    ILQR_TRY(pad_u(h, u, h->pu));
    if (x_traj) ILQR_TRY(pad_x(h, x_traj, h->pxt));
    // with a status array the inner call folds it (and synchronises)
    const ilqr_status bst = ilqr_backward_tracking(h->pad, &pp, o, h->px, h->pu, x_traj ? h->pxt : nullptr,
                                                   h->pd, h->pK, status);
    if (bst != ILQR_OK && bst != ILQR_ERR_NAN) return bst;
    ILQR_TRY(unpad_u(h, h->pd, d));
    ILQR_TRY(unpad3(h, h->pK, K, (size_t)h->batch * h->T, h->nu, h->nx, PAD_NU, PAD_NX));
    if (status) HIP_TRY(hipStreamSynchronize(h->stream));
    return bst;
  }
  if (two_link(p))
    HIP_TRY(ilqr::launch_tl_backward(ilqr::two_link_params(), h->nu, h->batch, h->T, x, u, h->J, d, K,
                                     status, ilqr::ls_params(o).mu, h->stream));
  else
    HIP_TRY(ilqr::launch_lq_backward(h->nx, h->nu, lq_params(p), h->batch, h->T, x, u, d, K,
                                     status, ilqr::ls_params(o).mu, h->stream, h->bw_wave, x_traj));
  if (status) HIP_TRY(ilqr::fold_status(status, h->batch, h->stream, h->host_status, &st));
  return st;
}

ilqr_status ilqr_backward_tiles(ilqr_handle* h, const ilqr_tiles* tl, const ilqr_options* o,
                                double* d, double* K, int32_t* status) {
  if (!h || !tl) return ILQR_ERR_BAD_ARG;
  ilqr_status st = ilqr::check_options(o);
  if (st != ILQR_OK) return st;
  if (!ilqr::tiles_supported(h->nx, h->nu)) return ILQR_ERR_UNSUPPORTED;
  if (!tl->A || !tl->B || !tl->lx || !tl->lu || !tl->lxx || !tl->luu || !tl->lfx || !tl->lfxx ||
      !d || !K)
    return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const ilqr::TileParams P{tl->A, tl->B, tl->lx, tl->lu, tl->lxx, tl->lux, tl->luu, tl->lfx, tl->lfxx};
  HIP_TRY(ilqr::launch_tiles_backward(h->nx, h->nu, P, h->batch, h->T, d, K, status,
                                      ilqr::ls_params(o).mu, h->stream));
  if (status) HIP_TRY(ilqr::fold_status(status, h->batch, h->stream, h->host_status, &st));
  return st;
}

ilqr_status ilqr_linearize(ilqr_handle* h, const ilqr_problem* p, const double* x, const double* u,
                           double* A, double* B) {
  const ilqr_status st = check_problem(h, p);
  if (st != ILQR_OK) return st;
  if (!A || !B) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(h->device));
  if (two_link(p)) {
    if (!x || !u) return ILQR_ERR_BAD_ARG;
    HIP_TRY(ilqr::launch_tl_jacobian(ilqr::two_link_params(), h->nu, h->batch, h->T, x, u, A, B, h->stream));
  } else {  // LQ of any supported or padded shape: the caller's (nx, nu) matrices as given
    HIP_TRY(ilqr::launch_lq_linearize(h->nx, h->nu, lq_params(p), h->batch, h->T, A, B, h->stream));
  }
  return ILQR_OK;
}

ilqr_status ilqr_forward(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                         const double* x, const double* u, const double* x_traj,
                         const double* d, const double* K, const double* prev_cost,
                         double* x_new, double* u_new, double* new_cost, int32_t* trials,
                         int32_t* status) {
  ilqr_status st = check_problem(h, p);
  if (st != ILQR_OK) return st;
  if ((st = ilqr::check_options(o)) != ILQR_OK) return st;
  if (!x || !u || !d || !K || !prev_cost || !x_new || !u_new || !new_cost) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(h->device));
  if (padded(h, p)) {
    ILQR_TRY(ensure_pad(h));
    ilqr_problem pp;
    ILQR_TRY(pad_problem(h, p, &pp));
    ILQR_TRY(pad_x(h, x, h->px));
    ILQR_TRY(pad_u(h, u, h->pu));
    if (x_traj) ILQR_TRY(pad_x(h, x_traj, h->pxt));
    ILQR_TRY(pad_u(h, d, h->pd));
    ILQR_TRY(pad3(h, K, h->pK, (size_t)h->batch * h->T, h->nu, h->nx, PAD_NU, PAD_NX));
    const ilqr_status fst = ilqr_forward(h->pad, &pp, o, h->px, h->pu, x_traj ? h->pxt : nullptr,
                                         h->pd, h->pK, prev_cost, h->pxn, h->pun, new_cost, trials,
                                         status);
    if (fst != ILQR_OK && fst != ILQR_ERR_NAN && fst != ILQR_ERR_LS_EXHAUSTED) return fst;
    ILQR_TRY(unpad_x(h, h->pxn, x_new));
    ILQR_TRY(unpad_u(h, h->pun, u_new));
    if (status) HIP_TRY(hipStreamSynchronize(h->stream));
    return fst;
  }
  if (two_link(p))
    HIP_TRY(ilqr::launch_tl_forward(ilqr::two_link_params(), h->nu, h->batch, h->T, x, u, x_traj, d, K,
                                    prev_cost, x_new, u_new, new_cost, trials, status,
                                    ilqr::ls_params(o), h->stream));
  else
    HIP_TRY(ilqr::launch_lq_forward(h->nx, h->nu, lq_params(p), h->batch, h->T, x, u, x_traj, d,
                                    K, prev_cost, x_new, u_new, new_cost, trials, status,
                                    ilqr::ls_params(o), h->stream, h->fw_ring, h->fw_mfma));
  if (status) HIP_TRY(ilqr::fold_status(status, h->batch, h->stream, h->host_status, &st));
  return st;
}

ilqr_status ilqr_iterate(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                         const double* x, const double* u, const double* x_traj, double* x_new,
                         double* u_new, const double* prev_cost, double* new_cost, double* du2,
                         int32_t* trials,
                         int32_t* status) {
  ilqr_status st = check_problem(h, p);
  if (st != ILQR_OK) return st;
  if ((st = ilqr::check_options(o)) != ILQR_OK) return st;
  if (!x || !u || !x_new || !u_new || !new_cost || !status) return ILQR_ERR_BAD_ARG;
  if ((st = check_tracking(h, p)) != ILQR_OK) return st;
  HIP_TRY(hipSetDevice(h->device));
  if (padded(h, p)) {
    ILQR_TRY(ensure_pad(h));
    ilqr_problem pp;
    ILQR_TRY(pad_problem(h, p, &pp));
    ILQR_TRY(pad_x(h, x, h->px));
    ILQR_TRY(pad_u(h, u, h->pu));
    if (x_traj) ILQR_TRY(pad_x(h, x_traj, h->pxt));
    ILQR_TRY(ilqr_iterate(h->pad, &pp, o, h->px, h->pu, x_traj ? h->pxt : nullptr, h->pxn, h->pun,
                          prev_cost, new_cost, du2, trials, status));
    ILQR_TRY(unpad_x(h, h->pxn, x_new));
    return unpad_u(h, h->pun, u_new);
  }
  h->reuse_valid = false;  // writes h->K: a fit's stored gains are gone
  ilqr::IterArgs a{};
  a.x = x;
  a.u = u;
  a.xtraj = x_traj;
  a.xnew = x_new;
  a.unew = u_new;
  a.K = h->K;
  a.d = h->d;
  a.prev_cost = prev_cost;
  a.new_cost = new_cost;
  a.du2 = du2;
  a.trials = trials;
  a.status = status;
  a.res_parity = nullptr;
  a.iters = nullptr;
  a.parity = 0;
  a.iter = 0;
  a.track = h->track;
  return enqueue_iteration(h, p, a, ilqr::ls_params(o), /*chain=*/false);
}

ilqr_status ilqr_fit(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                     const double* x_init, const double* u_init, const double* x_traj,
                     double* x_out, double* u_out, double* cost, int32_t* iters,
                     int32_t* status) {
  return ilqr_fit_ex(h, p, o, x_init, u_init, x_traj, x_out, u_out, cost, iters, status, nullptr);
}

ilqr_status ilqr_fit_ex(ilqr_handle* h, const ilqr_problem* p, const ilqr_options* o,
                        const double* x_init, const double* u_init, const double* x_traj,
                        double* x_out, double* u_out, double* cost, int32_t* iters,
                        int32_t* status, const ilqr_history* hist) {
  if (hist && !hist->cost && !hist->trials && !hist->alpha && !hist->du2) hist = nullptr;
  ilqr_status st = check_problem(h, p);
  if (st != ILQR_OK) return st;
  if ((st = ilqr::check_options(o)) != ILQR_OK) return st;
  if (!x_init || !u_init || !x_out || !u_out) return ILQR_ERR_BAD_ARG;
  if ((st = check_tracking(h, p)) != ILQR_OK) return st;
  ilqr_options def;
  ilqr_default_options(&def);
  if (!o) o = &def;
  HIP_TRY(hipSetDevice(h->device));
  if (padded(h, p)) {
    ILQR_TRY(ensure_pad(h));
    ilqr_problem pp;
    ILQR_TRY(pad_problem(h, p, &pp));
    ILQR_TRY(pad_x(h, x_init, h->px));
    ILQR_TRY(pad_u(h, u_init, h->pu));
    if (x_traj) ILQR_TRY(pad_x(h, x_traj, h->pxt));
    const ilqr_status fst = ilqr_fit_ex(h->pad, &pp, o, h->px, h->pu, x_traj ? h->pxt : nullptr,
                                        h->pxn, h->pun, cost, iters, status, hist);
    if (fst != ILQR_OK && fst != ILQR_ERR_NAN && fst != ILQR_ERR_LS_EXHAUSTED) return fst;
    ILQR_TRY(unpad_x(h, h->pxn, x_out));
    ILQR_TRY(unpad_u(h, h->pun, u_out));
    HIP_TRY(hipStreamSynchronize(h->stream));  // fit returns with its outputs written
    return fst;
  }
  hipStream_t s = h->stream;
  ilqr::FitState& f = h->fit;
  // the pipelined schedule interleaves two iterations per launch: a fit that records
  // its history runs the sequential schedule instead (the same bits)
  const bool pipe = !two_link(p) && h->pipelined && !hist;
  // the per-trajectory state is set by the first iteration's kernel itself on the fused
  // LQ path, else by fit_begin's launch
  const bool init_in_iter = fused_path(h, p) && !pipe && o->max_iter > 0;
  const ilqr::LSParams ls = ilqr::ls_params(o);
  // Gain reuse. Within the call (reuse_fit): iteration 1 stores the gains and the factor,
  // iterations ≥ 2 read them back (enqueue_iteration). Across calls (keep): they stay
  // valid for the next fit, whose iteration 1 then checks (check_now) on the device that
  // the operands are still the snapshot's, bit for bit — the caller may rewrite the problem
  // in place or hand over other buffers, so it is checked, never assumed. Valid means: left
  // by a fit on this path that returned without a HIP error, at this μ; every other writer
  // of K or fac clears it on entry, and so does this fit until it has returned. A fit
  // with max_iter = 0 launches no iteration and changes nothing.
  const bool reuse_fit = init_in_iter && !h->full_bw && h->fac;
  const bool keep = reuse_fit && !h->per_call && h->snap;
  if (o->max_iter > 0) {
    h->check_now = keep && h->reuse_valid && std::memcmp(&h->reuse_mu, &ls.mu, sizeof(double)) == 0;
    h->reuse_valid = false;
    h->branch_set = reuse_fit && h->branch;
  }
  ilqr::FitCall c;
  c.B = h->batch, c.T = h->T, c.nx = h->nx, c.nu = h->nu;
  c.max_iter = o->max_iter;
  c.x_init = x_init, c.u_init = u_init, c.x_out = x_out, c.u_out = u_out;
  for (int i = 0; i < 2; ++i) c.xbuf[i] = h->xbuf[i], c.ubuf[i] = h->ubuf[i];
  HIP_TRY(ilqr::fit_begin(f, c, x_traj, o->tol, /*init=*/!init_in_iter, s));
  auto iter_args = [&](int it) {
    const ilqr::FitBuffers b = ilqr::fit_buffers(c, it);
    ilqr::IterArgs a{};
    a.x = (const double*)b.x;
    a.u = (const double*)b.u;
    a.xtraj = x_traj;
    a.xnew = (double*)b.xnew;
    a.unew = (double*)b.unew;
    a.K = h->K;
    a.d = h->d;
    a.prev_cost = (const double*)f.prev_cost;  // in place: prev_cost = new_cost (:168)
    a.new_cost = (double*)f.prev_cost;
    a.du2 = (double*)f.du2;
    a.trials = f.trials;
    a.status = f.status;
    a.res_parity = f.res_parity;
    a.iters = f.iters;
    a.parity = b.parity;
    a.iter = it;
    a.init = init_in_iter && it == 1;
    a.track = h->track;
    // gain reuse (above): without `keep` no snapshot is written and nothing outlives the call
    a.fac = reuse_fit ? h->fac : nullptr;
    a.snap = keep ? h->snap : nullptr;
    a.branch = reuse_fit && it == 1 ? h->branch : nullptr;
    return a;
  };
  if (pipe) {
    // Launch `it` runs iteration it for role-B workgroups and forward(it−1) +
    // backward(it) for role A; launch max_iter+1 drains A's last forward.
    for (int it = 1; it <= o->max_iter + 1; ++it) {
      int flags = 0;
      if (it <= o->max_iter) flags |= ilqr::PIPE_A_BW_FLAG | ilqr::PIPE_B_FLAG;
      if (it >= 2) flags |= ilqr::PIPE_A_FW_FLAG;
      if (!flags) continue;
      HIP_TRY(ilqr::launch_lq_iter_pipe(h->nx, h->nu, lq_params(p), h->batch, h->T, iter_args(it),
                                        iter_args(it - 1), ls, flags, s));
    }
    c.enqueued = o->max_iter;
  }
  for (int it = 1; !pipe && it <= o->max_iter; ++it) {  // forward_pass.jl:161
    // iterations chain per chunk: chunk 0's next backward overlaps chunk 1's forward
    const ilqr_status st = enqueue_iteration(h, p, iter_args(it), ls, /*chain=*/true, hist);
    if (st != ILQR_OK) return st;
    // the history record and the count run behind every chunk's forward without
    // joining the main stream (a join would keep chunk 0's next backward from
    // overlapping chunk 1's forward): the forwards of all chunks are in order on the
    // side stream
    const hipStream_t ps = (two_link(p) || h->nchunks == 1) ? s : h->side;
    // (chunked: enqueue_iteration recorded each chunk right behind its forward)
    if (hist && ps == s)
      HIP_TRY(ilqr::launch_record_history(h->batch, it, f.status, f.iters, f.trials, f.prev_cost, f.du2, false,
                                          ls.alpha0, ls.shrink, hist->cost, hist->trials, hist->alpha,
                                          hist->du2, ps));
    bool stopped;
    HIP_TRY(ilqr::fit_poll(f, c, it, ps, &stopped));
    if (stopped) break;
  }
  ILQR_TRY(join(h, p));
  HIP_TRY(ilqr::fit_end(f, c, cost, iters, status, s, &st));
  if (keep) {  // every kernel of the fit has completed without a HIP error
    h->reuse_valid = true;
    h->reuse_mu = ls.mu;
  }
  return st;
}

ilqr_status ilqr_reuse_record(ilqr_handle* h, int32_t* out, int32_t capacity, int32_t* count) {
  if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return ILQR_ERR_BAD_ARG;
  if (h->pad && lq_paddable(h->nx, h->nu)) h = h->pad;  // a padded shape fits on its inner handle
  *count = 0;
  if (!h->branch_set) return ILQR_OK;
  HIP_TRY(hipSetDevice(h->device));
  const int32_t n = (int32_t)ilqr::lq_fused_waves((size_t)h->batch);
  const int32_t m = std::min(n, capacity);
  if (m > 0) {
    HIP_TRY(hipMemcpyAsync(out, h->branch, sizeof(int32_t) * m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  *count = n;
  return ILQR_OK;
}

ilqr_status ilqr_malloc(ilqr_handle* h, size_t bytes, void** ptr) {
  if (!h || !ptr) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMalloc(ptr, bytes));
  return ILQR_OK;
}

ilqr_status ilqr_free(ilqr_handle* h, void* ptr) {
  if (!h) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipFree(ptr));
  return ILQR_OK;
}

ilqr_status ilqr_memcpy_h2d(ilqr_handle* h, void* dst, const void* src, size_t bytes) {
  if (!h || !dst || !src) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ILQR_OK;
}

ilqr_status ilqr_memcpy_d2h(ilqr_handle* h, void* dst, const void* src, size_t bytes) {
  if (!h || !dst || !src) return ILQR_ERR_BAD_ARG;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ILQR_OK;
}

ilqr_status ilqr_selftest(int device, int32_t* failures) {
  const int f = ilqr::run_selftest(device);
  if (f < 0) {
    g_last_error = "selftest: HIP error";
    return ILQR_ERR_HIP;
  }
  if (failures) *failures = f;
  return ILQR_OK;
}

}  // extern "C"
