// api_util.h -- error plumbing and the owners of a device allocation (DevBuf) and of a list of events (EventList) shared by
// the extern "C" translation units.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/crispy_hip.h"

namespace crispy {

// Sets the calling thread's last-error message and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_error_cstr();
// CRISPY_OK if `device` is a usable gfx950 device, else an error with `who` in the message.
int check_device(int device, const char* who);
bool device_is_gfx950(int dev);
// Called from a catch (...) handler of an extern "C" entry point: classifies the exception in flight
// (std::bad_alloc / std::length_error -> CRISPY_ERR_OOM, anything else -> CRISPY_ERR_HIP), records a message and
// returns the status.  Never throws (the message buffer is a fixed thread-local array).
int fail_exception(const char* where) noexcept;

// Rust's str::trim(): Unicode White_Space off both ends of a UTF-8 string (the chunk texts of a recording, the words and
// the result of the diarized text).
bool unicode_space(unsigned cp);
std::string trim_unicode(const std::string& s);

// Environment variables the library reads -- two kinds, nothing else calls getenv:
//  * test hooks (test_env): read in every build and listed under "Environment" in include/crispy_hip.h.  They select
//    between forms that give bit-identical results (the tests that use them assert exactly that), never a result;
//  * developer knobs (dev_env): A/B switches for tools/ (ramps, request depths, timelines, tile walkers).  Compiled OUT of
//    the release library -- a host's environment must not steer which kernel form the product runs -- and in with
//    `make dev` (-DCRISPY_DEV_KNOBS, ../libcrispy_hip_dev.so; tools pick it through CRISPY_HIP_LIB).
inline const char* test_env(const char* name) { return std::getenv(name); }
#ifdef CRISPY_DEV_KNOBS
inline const char* dev_env(const char* name) { return std::getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

// A device allocation that belongs to its holder: freed with it (or when a fresh one is assigned over it), moved, never
// copied.  alloc replaces what it holds, grow only when that is too small -- neither carries the contents over.  After a
// failed alloc it holds nothing (bytes 0): the next call allocates again.  The holder's device must be current when one
// is let go.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr; bytes = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n);
    if (e == hipSuccess) bytes = n; else p = nullptr;
    return e;
  }
  hipError_t grow(size_t n) { return n <= bytes ? hipSuccess : alloc(n); }
  operator T*() const { return p; }
  template <class U> U* as() const { return reinterpret_cast<U*>(p); }      // the same bytes as another element type (the f16 caches)
};

// Events that belong to their holder: destroyed with it, never copied.  ensure(n, flags) creates what is missing up to n
// (flags as for hipEventCreateWithFlags; 0: events that can be timed).  The holder's device must be current when one is let go.
struct EventList {
  std::vector<hipEvent_t> v;
  EventList() = default;
  EventList(const EventList&) = delete;
  EventList& operator=(const EventList&) = delete;
  ~EventList() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
  hipError_t ensure(size_t n, unsigned flags) {
    while (v.size() < n) {
      hipEvent_t e;
      const hipError_t rc = hipEventCreateWithFlags(&e, flags);
      if (rc != hipSuccess) return rc;
      v.push_back(e);
    }
    return hipSuccess;
  }
  hipEvent_t operator[](size_t i) const { return v[i]; }
};

}  // namespace crispy

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return ::crispy::fail(_e == hipErrorOutOfMemory ? CRISPY_ERR_OOM : CRISPY_ERR_HIP, "%s: %s", #expr, \
                            hipGetErrorString(_e));                                                \
  } while (0)

// Every extern "C" definition is a function-try-block closed by one of these: nothing unwinds into the caller
// (the reference host builds with panic=abort, Cargo.toml:10-20; a C++ exception crossing the FFI is UB there).
#define CRISPY_CATCH_RET(name) catch (...) { return ::crispy::fail_exception(name); }
#define CRISPY_CATCH_VOID(name) catch (...) { (void)::crispy::fail_exception(name); }
