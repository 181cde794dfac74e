// Error reporting shared by all entry points of libdeepcam_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/deepcam_hip.h"

static thread_local char g_err[512] = "";

extern "C" const char* dc_last_error(void) { return g_err; }
extern "C" int dc_version(void) { return 1; }

extern "C" int dc_set_error(int code, const char* file, int line) {
  snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d", code, hipGetErrorString((hipError_t)code), file, line);
  return code ? code : -1;
}

extern "C" int dc_fail(const char* msg, const char* file, int line) {
  snprintf(g_err, sizeof(g_err), "%s (%s:%d)", msg, file ? file : "?", line);
  return -2;
}

extern "C" int dc_check_view(const void* ptr, int ld, int c, int dtype, const char* what) {
  const int es = dtype == DC_BF16 ? 2 : 4;
  const int kpv = 16 / es;
  const char* why = nullptr;
  if (ptr == nullptr) why = "null pointer";
  else if (((uintptr_t)ptr & 15) != 0) why = "pointer not 16-byte aligned";
  else if (c <= 0 || c % kpv != 0) why = "channel count not a positive multiple of the 16-byte vector";
  else if (ld < c || ld % kpv != 0) why = "pixel stride (ld) smaller than C or not vector aligned";
  if (why == nullptr) return 0;
  snprintf(g_err, sizeof(g_err), "%s: %s (ld=%d, C=%d, dtype=%d)", what, why, ld, c, dtype);
  return -3;
}

// ---- launch record: which kernel family served each call (tests).  Thread-local like the error string; the launch sites (DC_LAUNCHED,
// common.h) test g_launch_log_on and call launch_log_note with a string literal, so the record keeps pointers only.
namespace dc {
thread_local bool g_launch_log_on = false;
static constexpr int kLaunchLogCap = 4096;
static thread_local const char* g_launch_log[kLaunchLogCap];
static thread_local int g_launch_log_n = 0;            // launches noted since _begin (may exceed the capacity: overflow)
static thread_local bool g_launch_log_open = false;    // between _begin and _end (stays true when an overflow stopped the notes)
void launch_log_note(const char* name) {
  if (g_launch_log_n < kLaunchLogCap) g_launch_log[g_launch_log_n] = name;
  ++g_launch_log_n;
}
}  // namespace dc

extern "C" int dc_launch_log_begin(void) {
  if (dc::g_launch_log_open) return dc_fail("dc_launch_log_begin: a record is already open on this thread (dc_launch_log_end closes it)", __FILE__, __LINE__);
  dc::g_launch_log_open = dc::g_launch_log_on = true;
  dc::g_launch_log_n = 0;
  return 0;
}

extern "C" int dc_launch_log_end(char* buf, size_t cap) {
  if (!dc::g_launch_log_open) return dc_fail("dc_launch_log_end: no record is open on this thread (dc_launch_log_begin opens one)", __FILE__, __LINE__);
  dc::g_launch_log_open = dc::g_launch_log_on = false;      // whatever follows, the record is closed
  const int n = dc::g_launch_log_n;
  if (n > dc::kLaunchLogCap) {
    char msg[160];
    snprintf(msg, sizeof(msg), "dc_launch_log_end: %d launches overflowed the record of %d", n, dc::kLaunchLogCap);
    return dc_fail(msg, __FILE__, __LINE__);
  }
  size_t need = 1;
  for (int i = 0; i < n; ++i) need += strlen(dc::g_launch_log[i]) + (i ? 1 : 0);
  if (buf == nullptr || cap < need) {
    char msg[160];
    snprintf(msg, sizeof(msg), "dc_launch_log_end: the buffer holds %zu bytes, the record of %d launches needs %zu", buf ? cap : (size_t)0, n, need);
    return dc_fail(msg, __FILE__, __LINE__);
  }
  char* o = buf;
  for (int i = 0; i < n; ++i) {
    if (i) *o++ = '\n';
    const size_t l = strlen(dc::g_launch_log[i]);
    memcpy(o, dc::g_launch_log[i], l);
    o += l;
  }
  *o = 0;
  return 0;
}

// A non-blocking HIP stream at the lowest (level < 0), default (0) or highest (level > 0) priority the device offers.  The
// engine puts the weight-gradient work on a lowest-priority stream so that it fills the CUs the dependent backward chain
// leaves idle instead of competing with it workgroup for workgroup.
extern "C" int dc_stream_create(int level, void** stream) {
  if (stream == nullptr) return dc_fail("dc_stream_create: null argument", __FILE__, __LINE__);
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  const int prio = level < 0 ? least : (level > 0 ? greatest : 0);
  hipStream_t st = nullptr;
  e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio);
  if (e != hipSuccess) return dc_set_error(e, __FILE__, __LINE__);
  *stream = st;
  return 0;
}

extern "C" int dc_stream_destroy(void* stream) {
  if (stream == nullptr) return 0;
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? 0 : dc_set_error(e, __FILE__, __LINE__);
}

extern "C" int dc_stream_priority_range(int* least, int* greatest) {
  if (least == nullptr || greatest == nullptr) return dc_fail("dc_stream_priority_range: null argument", __FILE__, __LINE__);
  hipError_t e = hipDeviceGetStreamPriorityRange(least, greatest);
  return e == hipSuccess ? 0 : dc_set_error(e, __FILE__, __LINE__);
}
