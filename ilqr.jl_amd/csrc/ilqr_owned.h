// The one owner of a handle's device resources (host-only; no HIP types, so
// tests/test_owned.py compiles it with a host compiler and drives it with a counting fake).
//
// A handle holds one Owned by value and acquires its device buffers, pinned buffers, events
// and streams through it, in create or at a documented lazy first use. The
// owner is a list and a sticky error, nothing more:
//   * a required request (dev, dev_zero, pinned, event, stream) after the first failure is a
//     no-op, and error() keeps that first failure: the `if (e == ok) e = alloc(...)` chain;
//   * an optional request (try_dev) that fails leaves its pointer null, clears the runtime's
//     last error and does not poison the owner; the caller drops the partners with drop();
//   * release() frees everything in reverse order of acquisition, each object once, writes
//     null back through every pointer it was given, and clears the error: the owner can be
//     filled again from nothing. The destructor releases.
// What is freed is what the registered pointer holds at release (a handle may swap two of its
// own buffers). `Api` is the runtime: HipApi (ilqr_internal.h), or a test's fake.
#pragma once
#include <cstddef>
#include <type_traits>
#include <vector>

namespace ilqr {

template <class Api>
class Owned {
 public:
  using Error = typename Api::Error;
  using Event = typename Api::Event;
  using Stream = typename Api::Stream;
  static_assert(std::is_pointer<Event>::value && std::is_pointer<Stream>::value, "events and streams are pointers");

  explicit Owned(Api api = Api{}) : api_(api) {}
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { release(); }

  void set_device(int device) { device_ = device; }
  Error error() const { return err_; }
  bool ok() const { return err_ == Api::ok; }

  // `count` elements of T (bytes for a void*)
  template <class T>
  void dev(T** p, size_t count) {
    acquire(DEV, p, [&] { return api_.dev_alloc((void**)p, bytes<T>(count)); });
  }
  template <class T>
  void dev_zero(T** p, size_t count) {
    dev(p, count);
    if (ok()) err_ = api_.dev_zero(*p, bytes<T>(count));
  }
  template <class T>
  bool try_dev(T** p, size_t count) {
    *p = nullptr;
    if (!ok()) return false;
    if (api_.dev_alloc((void**)p, bytes<T>(count)) == Api::ok) {
      items_.push_back({DEV, (void**)p});
      return true;
    }
    *p = nullptr;
    api_.clear_last_error();
    return false;
  }
  template <class T>
  void pinned(T** p, size_t count, unsigned flags) {
    acquire(PINNED, p, [&] { return api_.pinned_alloc((void**)p, bytes<T>(count), flags); });
  }
  void event(Event* p, unsigned flags) {
    acquire(EVENT, p, [&] { return api_.event_create(p, flags); });
  }
  void stream(Stream* p, unsigned flags) {
    acquire(STREAM, p, [&] { return api_.stream_create(p, flags); });
  }

  // release one buffer early (the partner of a failed try_dev); null or unknown: nothing
  template <class T>
  void drop(T** p) {
    for (size_t i = items_.size(); i-- > 0;)
      if (items_[i].slot == (void**)p) {
        if (*p) api_.set_device(device_);
        free_item(items_[i]);
        items_.erase(items_.begin() + i);
      }
  }

  void release() {
    if (!items_.empty()) api_.set_device(device_);
    for (size_t i = items_.size(); i-- > 0;) free_item(items_[i]);
    items_.clear();
    err_ = Api::ok;
  }

 private:
  enum Kind { DEV, PINNED, EVENT, STREAM };
  struct Item {
    Kind kind;
    void** slot;
  };
  template <class T>
  static size_t bytes(size_t count) {
    return count * sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);
  }
  template <class P, class F>
  void acquire(Kind k, P* p, F make) {
    if (!ok()) return;
    *p = nullptr;
    if ((err_ = make()) == Api::ok)
      items_.push_back({k, (void**)p});
    else
      *p = nullptr;
  }
  void free_item(const Item& it) {
    void* q = *it.slot;
    *it.slot = nullptr;
    if (!q) return;
    switch (it.kind) {
      case DEV: api_.dev_free(q); break;
      case PINNED: api_.pinned_free(q); break;
      case EVENT: api_.event_destroy((Event)q); break;
      case STREAM: api_.stream_destroy((Stream)q); break;
    }
  }

  Api api_;
  int device_ = 0;
  Error err_ = Api::ok;
  std::vector<Item> items_;
};

}  // namespace ilqr
