// CPU driver of tests/test_owned.py: ilqr_owned.h (the owner of a handle's device resources)
// instantiated with a counting fake runtime. The fake hands out distinct tokens, records every
// acquire and release with its kind, and fails the k-th acquisition on request. Built with
// -fsanitize=address,undefined and run with leak checking on; prints one line per scenario,
// "<name> ok" or "<name> FAIL <what>", and exits 1 if any failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "ilqr_owned.h"

namespace {

enum Kind { DEV, PINNED, EVENT, STREAM };

struct Ledger {
  int attempts = 0;  // acquisitions asked of the runtime
  int fail_at = 0;   // the attempt that fails (1-based; 0: none)
  bool fail_zero = false;
  bool last_error = false;  // the runtime's sticky last-error flag
  std::vector<uintptr_t> acquired, released, zeroed;
  std::map<uintptr_t, Kind> kind;
  std::vector<int> devices;  // every set_device
  std::string wrong;         // a release of the wrong kind, of an unknown token, or twice

  static int code(int k) { return 100 + k; }
  int acquire(void** p, Kind k) {
    ++attempts;
    if (attempts == fail_at) {
      last_error = true;
      *p = (void*)(uintptr_t)0xdead;  // a runtime may scribble on failure
      return code(attempts);
    }
    const uintptr_t t = 0x1000 + 0x40 * (uintptr_t)attempts;
    acquired.push_back(t);
    kind[t] = k;
    *p = (void*)t;
    return 0;
  }
  void release(void* p, Kind k) {
    const uintptr_t t = (uintptr_t)p;
    if (!kind.count(t) || kind[t] != k) wrong += " kind/unknown:" + std::to_string(t);
    if (std::count(released.begin(), released.end(), t)) wrong += " twice:" + std::to_string(t);
    released.push_back(t);
  }
};

struct FakeEvent;
struct FakeStream;
struct FakeApi {
  using Error = int;
  using Event = FakeEvent*;
  using Stream = FakeStream*;
  static constexpr int ok = 0;
  Ledger* L = nullptr;
  int dev_alloc(void** p, size_t) { return L->acquire(p, DEV); }
  int dev_zero(void* p, size_t) {
    L->zeroed.push_back((uintptr_t)p);
    return L->fail_zero ? 7 : 0;
  }
  void dev_free(void* p) { L->release(p, DEV); }
  int pinned_alloc(void** p, size_t, unsigned) { return L->acquire(p, PINNED); }
  void pinned_free(void* p) { L->release(p, PINNED); }
  int event_create(Event* e, unsigned) { return L->acquire((void**)e, EVENT); }
  void event_destroy(Event e) { L->release(e, EVENT); }
  int stream_create(Stream* s, unsigned) { return L->acquire((void**)s, STREAM); }
  void stream_destroy(Stream s) { L->release(s, STREAM); }
  void set_device(int d) { L->devices.push_back(d); }
  void clear_last_error() { L->last_error = false; }
};
using Owner = ilqr::Owned<FakeApi>;

// a handle of ilqr_create's shape: required buffers, a zeroed one, a pinned one, two events, a
// stream, and two optional groups with a partner each
struct Handle {
  double *xbuf = nullptr, *ubuf = nullptr, *K = nullptr, *J = nullptr;
  void* raw = nullptr;  // sized in bytes
  int32_t *words = nullptr, *flags = nullptr;
  FakeEvent *ev0 = nullptr, *ev1 = nullptr;
  FakeStream* side = nullptr;
  double *sx = nullptr, *su = nullptr;              // optional group 1
  double* fac = nullptr;                            // optional group 2: snap and branch need fac
  double* snap = nullptr;
  int32_t* branch = nullptr;
  bool scratch = false, reuse = false, optional_failed = false;
  bool all_null() const {
    return !xbuf && !ubuf && !K && !J && !raw && !words && !flags && !ev0 && !ev1 && !side && !sx && !su && !fac &&
           !snap && !branch;
  }
};
constexpr int PLAN_STEPS = 15;  // acquisitions of a plan in which nothing fails

void plan(Owner& own, Handle& h) {
  own.set_device(3);
  own.dev(&h.xbuf, 100);                                           // 1
  own.dev(&h.ubuf, 40);                                            // 2
  own.dev(&h.raw, 64);                                             // 3
  own.pinned(&h.words, 4, 0x6);                                    // 4
  own.dev_zero(&h.flags, 2);                                       // 5
  own.event(&h.ev0, 2);                                            // 6
  own.event(&h.ev1, 2);                                            // 7
  own.dev(&h.K, 400);                                              // 8
  h.scratch = own.try_dev(&h.sx, 1000) && own.try_dev(&h.su, 500);  // 9, 10
  if (!h.scratch) {
    h.optional_failed |= own.ok();
    own.drop(&h.sx);
  }
  h.reuse = own.try_dev(&h.fac, 300);                              // 11
  if (!h.reuse) h.optional_failed |= own.ok();
  if (h.reuse && !(own.try_dev(&h.snap, 200) && own.try_dev(&h.branch, 8))) {  // 12, 13
    h.optional_failed |= own.ok();
    own.drop(&h.snap);
    h.reuse = false;
  }
  own.dev(&h.J, 50);                                               // 14
  own.stream(&h.side, 1);                                          // 15
}

int fails = 0;
void report(const std::string& name, const std::string& what) {
  if (what.empty()) {
    std::printf("%s ok\n", name.c_str());
  } else {
    std::printf("%s FAIL %s\n", name.c_str(), what.c_str());
    ++fails;
  }
}

// after release(): every token released once, with its own kind; those still held at the
// release come back in reverse order of acquisition; every pointer null; the device set
std::string check_released(const Ledger& L, const Handle& h, size_t released_before) {
  std::string bad = L.wrong;
  std::vector<uintptr_t> a = L.acquired, r = L.released;
  std::sort(a.begin(), a.end());
  std::sort(r.begin(), r.end());
  if (a != r) bad += " released set != acquired set";
  std::vector<uintptr_t> held;
  for (uintptr_t t : L.acquired)
    if (!std::count(L.released.begin(), L.released.begin() + released_before, t)) held.push_back(t);
  std::reverse(held.begin(), held.end());
  if (held != std::vector<uintptr_t>(L.released.begin() + released_before, L.released.end()))
    bad += " not in reverse order of acquisition";
  if (!h.all_null()) bad += " a registered pointer is not null";
  for (int d : L.devices)
    if (d != 3) bad += " wrong device";
  if (!held.empty() && L.devices.empty()) bad += " device not set before the release";
  return bad;
}

// failing acquisition k, every k of the plan
void sweep() {
  for (int k = 1; k <= PLAN_STEPS; ++k) {
    Ledger L;
    L.fail_at = k;
    Handle h;
    std::string bad;
    {
      Owner own(FakeApi{&L});
      plan(own, h);
      if (h.optional_failed != (k >= 9 && k <= 13)) bad += " the plan's steps 9 to 13, and no others, are optional";
      if (h.optional_failed) {  // the failure was an optional request: the owner stays usable
        if (!own.ok()) bad += " optional failure poisoned the owner";
        if (L.last_error) bad += " optional failure left the runtime's last error set";
        if (!h.J || !h.side) bad += " required requests after an optional failure did not succeed";
        if (h.scratch && h.reuse) bad += " no group was dropped";
        if (!h.scratch && (h.sx || h.su)) bad += " scratch partner kept";
        if (!h.reuse && (h.snap || h.branch)) bad += " reuse partner kept";
      } else {
        if (own.error() != Ledger::code(k)) bad += " error() is not the first failure";
        if (L.attempts != k) bad += " an acquisition was attempted after the failure";
      }
      const size_t before = L.released.size();
      own.release();
      bad += check_released(L, h, before);
      if (!own.ok()) bad += " release() kept the error";
      const size_t n = L.released.size(), nd = L.devices.size();
      own.release();
      if (L.released.size() != n || L.devices.size() != nd) bad += " a second release() released something";
    }
    report("fail_at_" + std::to_string(k), bad);
  }
}

void no_failure() {
  Ledger L;
  Handle h;
  std::string bad;
  Owner own(FakeApi{&L});
  plan(own, h);
  if (!own.ok() || L.attempts != PLAN_STEPS || (int)L.acquired.size() != PLAN_STEPS) bad += " plan did not complete";
  if (h.all_null() || !h.scratch || !h.reuse) bad += " pointers not set";
  if (L.zeroed != std::vector<uintptr_t>{(uintptr_t)h.flags}) bad += " dev_zero did not zero its buffer alone";
  own.release();
  bad += check_released(L, h, 0);
  report("no_failure", bad);
}

// a handle may swap two of its own buffers (a warm start swaps input and result): what a
// registered pointer holds at the release is what is freed, each token still once
void swapped() {
  Ledger L;
  Handle h;
  std::string bad;
  Owner own(FakeApi{&L});
  plan(own, h);
  std::swap(h.xbuf, h.K);
  own.release();
  std::vector<uintptr_t> a = L.acquired, r = L.released;
  std::sort(a.begin(), a.end());
  std::sort(r.begin(), r.end());
  if (a != r || !h.all_null()) bad += " swapped buffers not released once each";
  report("swapped", bad + L.wrong);
}

// the memset of dev_zero fails: the buffer is owned (and released), the error kept
void zero_failure() {
  Ledger L;
  L.fail_zero = true;
  Handle h;
  std::string bad;
  Owner own(FakeApi{&L});
  plan(own, h);
  if (own.error() != 7 || L.attempts != 5) bad += " the memset's failure did not stop the chain";
  own.release();
  bad += check_released(L, h, 0);
  report("zero_failure", bad);
}

// try_dev and drop alone
void optional() {
  Ledger L;
  std::string bad;
  double *a = nullptr, *b = nullptr, *c = nullptr;
  Owner own(FakeApi{&L});
  own.set_device(3);
  if (!own.try_dev(&a, 10)) bad += " try_dev failed without a failure";
  L.fail_at = 2;
  if (own.try_dev(&b, 10)) bad += " failed try_dev returned true";
  if (b) bad += " failed try_dev left its pointer set";
  if (L.last_error) bad += " last error not cleared";
  if (!own.ok()) bad += " owner poisoned";
  const uintptr_t ta = (uintptr_t)a;
  own.drop(&a);
  if (a || L.released != std::vector<uintptr_t>{ta}) bad += " drop did not release the partner once and null it";
  own.drop(&a);  // nothing left to drop
  own.drop(&b);
  if (L.released.size() != 1) bad += " drop of a null pointer released something";
  own.dev(&c, 10);
  if (!own.ok() || !c) bad += " required request after the failure did not succeed";
  own.release();
  if (L.released.size() != 2 || c) bad += " release after drop";
  bad += L.wrong;
  report("optional", bad);
}

// ensure_pad's pattern: a group that fails midway is released and filled again from nothing
void refill() {
  Ledger L;
  std::string bad;
  double* q[6] = {};
  Owner own(FakeApi{&L});
  own.set_device(3);
  L.fail_at = 4;
  for (double*& p : q) own.dev(&p, 16);
  if (own.ok() || L.attempts != 4) bad += " first fill did not fail at 4";
  own.release();
  for (double* p : q)
    if (p) bad += " pointer kept after the failed fill's release";
  if (L.released.size() != 3) bad += " failed fill's buffers not released";
  for (double*& p : q) own.dev(&p, 16);
  if (!own.ok()) bad += " second fill failed";
  for (double* p : q)
    if (!p || std::count(L.released.begin(), L.released.end(), (uintptr_t)p)) bad += " second fill's token not live";
  own.release();
  if (L.released.size() != 9) bad += " second fill not released";
  bad += L.wrong;
  report("refill", bad);
}

// no explicit release(): the destructor releases; the ledger is read after the scope
void destructor() {
  Ledger L;
  Handle h;
  {
    Owner own(FakeApi{&L});
    plan(own, h);
  }
  report("destructor", (int)L.released.size() == PLAN_STEPS ? check_released(L, h, 0) : " not everything released");
}

}  // namespace

int main() {
  sweep();
  no_failure();
  swapped();
  zero_failure();
  optional();
  refill();
  destructor();
  return fails ? 1 : 0;
}
