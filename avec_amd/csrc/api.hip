// Error plumbing + version for libavec_hip.so
#include "common.h"
#include "avec_hip.h"
#include "vec.h"
#include "host_tables.h"
#include <stdarg.h>
#include <stdio.h>

static thread_local char g_err[512] = "";

void avec_set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* avec_last_error() { return g_err; }

// name of the kernel instance the last GEMM-family entry point launched on this thread (bench.py's per-kernel roofline rows use it as the key)
static thread_local char g_kname[128] = "";
void avec_note_kernel(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_kname, sizeof(g_kname), fmt, ap); va_end(ap);
}
extern "C" const char* avec_last_kernel() { return g_kname; }
extern "C" int avec_version() { return AVEC_ABI_VERSION; }
extern "C" int avec_struct_size(int which) {
  switch (which) {
    case 0: return (int)sizeof(avec_rows_t); case 1: return (int)sizeof(avec_epilogue_t); case 2: return (int)sizeof(avec_attn_t); case 3: return (int)sizeof(avec_tn_item_t);
    case 4: return (int)sizeof(avec_tn_batched_t); case 5: return (int)sizeof(avec_ln_item_t); case 6: return (int)sizeof(avec_fp8_item_t); case 7: return (int)sizeof(avec_wgrad3x3_item_t);
    case 8: return (int)sizeof(avec_ngram_t);
    default: return -1;
  }
}

// ---------------------------------------------------------------------------------------------
// reduction workspace (vec.h: two-pass column reductions) and dynamic-LDS opt-in: the bookkeeping is host_tables.h, this file adds the current device and the HIP call
// ---------------------------------------------------------------------------------------------
static WsRegistry g_ws;
static LdsOptin g_lds;

extern "C" int avec_set_reduce_workspace(void* base, long long bytes) {
  int dev = 0; hipError_t e = hipGetDevice(&dev);
  AVEC_CHECK_ARG(e == hipSuccess && dev >= 0 && dev < WsRegistry::MAX_DEV, "set_reduce_workspace: no current device");
  AVEC_CHECK_ARG((base == nullptr && bytes == 0) || (base != nullptr && bytes >= (1 << 16) && ((size_t)base & 255) == 0),
                 "set_reduce_workspace: need a 256-byte aligned buffer of at least 64 KB (or NULL, 0 to unregister)");
  g_ws.set_default(dev, base, (size_t)bytes);
  return 0;
}
extern "C" int avec_set_reduce_workspace_stream(void* base, long long bytes, hipStream_t stream) {
  int dev = 0; hipError_t e = hipGetDevice(&dev);
  AVEC_CHECK_ARG(e == hipSuccess && dev >= 0 && dev < WsRegistry::MAX_DEV && base != nullptr && bytes >= (1 << 16) && ((size_t)base & 255) == 0, "set_reduce_workspace_stream: bad arguments");
  AVEC_CHECK_ARG(g_ws.set_stream(dev, stream, base, (size_t)bytes), "set_reduce_workspace_stream: at most %d stream-bound workspaces", WsRegistry::MAX_STREAMS);
  return 0;
}
ColWs avec_reduce_ws(size_t partial_floats, hipStream_t st) {
  int dev = 0; if (hipGetDevice(&dev) != hipSuccess) return ColWs{nullptr};
  return ColWs{(float*)g_ws.find(dev, st, partial_floats * sizeof(float))};
}

// 0, LdsOptin::TOO_LARGE, or the HIP error code of the refusal (hipErrorNoDevice without a current device)
int avec_lds_optin_quiet(const void* kernel, size_t bytes) {
  if (bytes <= LdsOptin::FREE_BYTES) return 0;
  int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0) return (int)hipErrorNoDevice;
  return g_lds.request(dev, kernel, bytes, [](const void* k, size_t n) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n);
    if (e != hipSuccess) (void)hipGetLastError();      // the refusal is reported by value; the next launch check must not see it
    return (int)e;
  });
}
int avec_lds_optin(const void* kernel, size_t bytes) {
  const int r = avec_lds_optin_quiet(kernel, bytes);
  if (r == LdsOptin::TOO_LARGE) avec_set_error("%zu bytes of LDS requested (> 160 KiB)", bytes);
  else if (r) avec_set_error("cannot reserve %zu bytes of LDS: %s", bytes, hipGetErrorString((hipError_t)r));
  return r;
}
