// The fit driver the LQ family (ilqr_abi.cpp), the chain family (ilqr_chain.hip) and the
// floating-base family (ilqr_floating.hip) share
// (src/forward_pass.jl:148-179, DESIGN.md §4 fit driver). Host code only. A handle holds one
// FitState; a fit call fills a FitCall and runs
//
//   fit_begin(f, c, ...);
//   for (it = 1 .. c.max_iter) {
//     b = fit_buffers(c, it);  <enqueue the family's own iteration on b>
//     fit_poll(f, c, it, stream, &stopped);  if (stopped) break;
//   }
//   fit_end(f, c, ...);
//
// Every function returns the first HIP error; the caller wraps it in its own error macro.
#pragma once
#include "ilqr_internal.h"

namespace ilqr {

// Per-trajectory fit state and the words the host and the device exchange during a fit.
struct FitState {
  void* prev_cost = nullptr;  // (B) of the family's value type (fp64, or the chain family's fp32)
  void* du2 = nullptr;        // (B) likewise
  int32_t* trials = nullptr;
  int32_t* status = nullptr;
  int32_t* res_parity = nullptr;
  int32_t* iters = nullptr;
  // host-mapped words: [0], [1] the running-trajectory counts of the convergence poll's last
  // two iterations, each behind an event; [2] the call status (gather_kernel: bit 0 NaN,
  // bit 1 exhausted line search) tagged with the fit's number
  int32_t* host_words = nullptr;
  int32_t* dev_words = nullptr;  // device alias of host_words
  int32_t* dev_flags = nullptr;  // gather_kernel's two device call-status words
  hipEvent_t ev_poll[2] = {nullptr, nullptr};
  HostWait host_wait;     // the end-of-fit wait (wait_host_seq)
  HostWait poll_wait;     // the per-iteration convergence polls (wait_event)
  uint32_t fit_seq = 0;   // fits so far (tags the host call-status word)
};

// `elem`: bytes of one cost value (4 or 8). Everything is acquired through the handle's owner
// (which releases it); the owner's first error, or the device alias's, is returned.
inline hipError_t fit_state_create(FitState* f, HipOwned& own, size_t B, size_t elem) {
  own.dev(&f->prev_cost, elem * B);
  own.dev(&f->du2, elem * B);
  for (int32_t** p : {&f->trials, &f->status, &f->res_parity, &f->iters}) own.dev(p, B);
  own.pinned(&f->host_words, 4, hipHostMallocMapped | hipHostMallocCoherent);
  own.dev_zero(&f->dev_flags, 2);
  for (hipEvent_t& ev : f->ev_poll) own.event(&ev, hipEventDisableTiming);
  if (!own.ok()) return own.error();
  return hipHostGetDevicePointer((void**)&f->dev_words, f->host_words, 0);
}

// One fit call. The caller fills the first block; fit_begin sets the second.
struct FitCall {
  int B = 0, T = 0, nx = 0, nu = 0;
  bool f32 = false;  // value type of every trajectory and cost array
  int max_iter = 0;
  const void *x_init = nullptr, *u_init = nullptr;
  void *x_out = nullptr, *u_out = nullptr;
  void* xbuf[2] = {nullptr, nullptr};  // the handle's ping-pong trajectories
  void* ubuf[2] = {nullptr, nullptr};

  bool direct = false;  // the last iteration writes x_out / u_out itself
  bool poll = false;    // the loop stops enqueueing once every trajectory has stopped
  int enqueued = 0, waited = 0;  // iterations (the end-of-fit wait's units)
};

// Where iteration `it` reads and writes, and the code of its input for res_parity.
struct FitBuffers {
  const void *x, *u;
  void *xnew, *unew;
  int parity;
};

// Clears the call-status word, sets the per-trajectory state (prev_cost = Inf,
// forward_pass.jl:159, status OK, result "the input", iterations 0) unless the first
// iteration's kernel does (`init` false), and decides `direct` and `poll`.
// The last iteration writes the caller's x_out / u_out directly (the gather then copies
// only trajectories that stopped earlier) unless they overlap an input.
inline hipError_t fit_begin(FitState& f, FitCall& c, const void* x_traj, double tol, bool init, hipStream_t s) {
  if (init) {
    const hipError_t e = launch_fit_init(c.B, f.prev_cost, c.f32, f.status, f.res_parity, f.iters, s);
    if (e != hipSuccess) return e;
  }
  *(volatile int32_t*)(f.host_words + 2) = 0;
  const size_t w = c.f32 ? 4 : 8;
  const size_t xb = w * (size_t)c.B * (c.T + 1) * c.nx, ub = w * (size_t)c.B * c.T * c.nu;
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = (const char*)a, *pb = (const char*)b;
    return b && pa < pb + nb && pb < pa + na;
  };
  c.direct = c.max_iter > 0 && !overlap(c.x_out, xb, c.x_init, xb) && !overlap(c.x_out, xb, x_traj, xb) &&
             !overlap(c.u_out, ub, c.u_init, ub) && !overlap(c.x_out, xb, c.u_init, ub) &&
             !overlap(c.u_out, ub, c.x_init, xb) && !overlap(c.u_out, ub, x_traj, xb);
  // With a convergence test (tol ≥ 0) the loop stops enqueueing once every trajectory has
  // stopped, like the reference's `break` (:171); see fit_poll.
  c.poll = tol >= 0.0 && c.max_iter > 2;
  c.enqueued = c.waited = 0;
  return hipSuccess;
}

// Iteration `it` reads x̄ⁱ (the caller's x_init / u_init for it = 1, no copy; else the
// handle's buffer (it−1)&1) and writes buffer it&1 (x̄ⁱ, ūⁱ = x̄ⁱ⁺¹, ūⁱ⁺¹, :174-175), the
// direct last one x_out / u_out. `parity` records where a trajectory's result lies when
// it stops in this iteration: PARITY_INPUT for the caller's buffers.
inline FitBuffers fit_buffers(const FitCall& c, int it) {
  const int par = (it - 1) & 1;
  const bool last = c.direct && it == c.max_iter;
  return FitBuffers{it == 1 ? c.x_init : c.xbuf[par], it == 1 ? c.u_init : c.ubuf[par],
                    last ? c.x_out : c.xbuf[par ^ 1], last ? c.u_out : c.ubuf[par ^ 1],
                    it == 1 ? PARITY_INPUT : par};
}

// After iteration `it` is enqueued: a one-block kernel on `s` (the stream the iteration's
// forward ran on) writes the running count to host-mapped memory behind an event, and the
// host reads iteration it−1's count while the GPU runs iteration it (no idle gap; at most
// one iteration of already-stopped waves is enqueued past the last useful one).
// *stopped: every trajectory had stopped after iteration it−1.
inline hipError_t fit_poll(FitState& f, FitCall& c, int it, hipStream_t s, bool* stopped) {
  *stopped = false;
  c.enqueued = it;
  if (!c.poll || it == c.max_iter) return hipSuccess;
  hipError_t e = launch_count_running(c.B, f.status, f.dev_words + (it & 1), s);
  if (e == hipSuccess) e = hipEventRecord(f.ev_poll[it & 1], s);
  if (e != hipSuccess || it < 2) return e;
  if ((e = wait_event(f.ev_poll[(it - 1) & 1], &f.poll_wait)) != hipSuccess) return e;
  c.waited = it - 1;
  *stopped = __atomic_load_n(f.host_words + ((it - 1) & 1), __ATOMIC_ACQUIRE) == 0;
  return hipSuccess;
}

// The end of a fit: the gather (still-running trajectories, max_iter reached, return the
// last accepted iterate: the one the last iteration wrote, the input when max_iter = 0),
// the launch that publishes the call status under this fit's number, and the host's wait
// for that word. *call: the call status.
inline hipError_t fit_end(FitState& f, const FitCall& c, void* cost, int32_t* iters, int32_t* status,
                          hipStream_t s, ilqr_status* call) {
  const int last = c.max_iter == 0 ? PARITY_INPUT : (c.direct ? PARITY_OUT : (c.max_iter & 1));
  uint32_t seq = (++f.fit_seq) & 0x3fffffffu;
  if (seq == 0) seq = f.fit_seq = 1;  // 0 is the word's cleared value
  hipError_t e = launch_gather_result(c.B, c.T, c.nx, c.nu, c.f32, c.x_init, c.u_init, c.xbuf[0], c.ubuf[0],
                                      c.xbuf[1], c.ubuf[1], f.res_parity, f.status, last, f.prev_cost, f.iters,
                                      c.x_out, c.u_out, cost, iters, status, f.dev_flags, f.dev_words + 2, s, seq);
  if (e == hipSuccess) e = wait_host_seq(f.host_words + 2, seq, c.enqueued - c.waited, s, &f.host_wait);
  if (e != hipSuccess) return e;
  *call = call_status(__atomic_load_n(f.host_words + 2, __ATOMIC_ACQUIRE));
  return hipSuccess;
}

}  // namespace ilqr
