// api_util.cpp -- thread-local error message and device checks shared by the C ABI.
#include "api_util.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>

namespace crispy {

namespace {
// fixed storage: recording an error must not allocate (it is what runs after a std::bad_alloc)
thread_local char g_last_error[768] = "";
}

int fail(int code, const char* fmt, ...) {
  char buf[sizeof(g_last_error)];      // fmt's arguments may point into g_last_error ("%s" of the previous message)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  std::memcpy(g_last_error, buf, sizeof(buf));
  return code;
}

const char* last_error_cstr() { return g_last_error; }

int fail_exception(const char* where) noexcept {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    return fail(CRISPY_ERR_OOM, "%s: host allocation failed (std::bad_alloc)", where);
  } catch (const std::length_error& e) {
    return fail(CRISPY_ERR_OOM, "%s: %s (std::length_error)", where, e.what());
  } catch (const std::exception& e) {
    return fail(CRISPY_ERR_HIP, "%s: unexpected C++ exception: %s", where, e.what());
  } catch (...) {
    return fail(CRISPY_ERR_HIP, "%s: unexpected non-standard C++ exception", where);
  }
}

bool device_is_gfx950(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
  return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

int check_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CRISPY_ERR_NO_DEVICE, "%s: no HIP device (this library has no CPU path)", who);
  if (device < 0 || device >= ndev)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: device %d out of range [0,%d)", who, device, ndev);
  if (!device_is_gfx950(device)) return fail(CRISPY_ERR_NO_DEVICE, "%s: device %d is not gfx950 (MI355X)", who, device);
  return CRISPY_OK;
}

// Rust's str::trim(): the code points with the White_Space property, off both ends of a UTF-8 string
// (managers/transcription.rs:187 trims every chunk's text; commands/transcription.rs:276 tests `trim().is_empty()`;
// managers/diarization.rs:674, 699 trim every word and the diarized text)
bool unicode_space(unsigned cp) {
  return (cp >= 9 && cp <= 13) || cp == 0x20 || cp == 0x85 || cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) ||
         cp == 0x2028 || cp == 0x2029 || cp == 0x202F || cp == 0x205F || cp == 0x3000;
}
std::string trim_unicode(const std::string& s) {
  auto decode = [&](size_t i, size_t* len) -> unsigned {      // one code point at byte i (malformed bytes stand for themselves)
    const unsigned char c = (unsigned char)s[i];
    auto cont = [&](size_t k) { return i + k < s.size() && ((unsigned char)s[i + k] & 0xC0) == 0x80; };
    if (c < 0x80) { *len = 1; return c; }
    if ((c & 0xE0) == 0xC0 && cont(1)) { *len = 2; return ((c & 0x1Fu) << 6) | ((unsigned char)s[i + 1] & 0x3Fu); }
    if ((c & 0xF0) == 0xE0 && cont(1) && cont(2)) {
      *len = 3;
      return ((c & 0x0Fu) << 12) | (((unsigned char)s[i + 1] & 0x3Fu) << 6) | ((unsigned char)s[i + 2] & 0x3Fu);
    }
    *len = 1;
    return 0xFFFFFFFFu;
  };
  size_t a = 0, b = s.size();
  while (a < b) {
    size_t len = 1;
    if (!unicode_space(decode(a, &len))) break;
    a += len;
  }
  while (b > a) {
    size_t k = b - 1;
    while (k > a && ((unsigned char)s[k] & 0xC0) == 0x80 && b - k < 3) --k;      // back to the lead byte of the last code point
    size_t len = 1;
    const unsigned cp = decode(k, &len);
    if (k + len != b || !unicode_space(cp)) break;
    b = k;
  }
  return s.substr(a, b - a);
}

}  // namespace crispy
