// error.cpp -- the library's process-wide state: thread-local last-error string, version, the per-device dynamic-LDS grants, and the load-time table of
// runtime switches (see include/deepliif_hip.h)
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <mutex>
#include <utility>
#include "../../include/deepliif_hip.h"
#include "switches.h"

static thread_local char g_err[512] = "";

void dl_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *dl_last_error(void) { return g_err; }

// ---- the dynamic-LDS grant (common.h).  hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel ON A DEVICE, and operands may live on any
// device of the process (the caller makes theirs current before it launches), so what has been granted is remembered per (device, kernel) -- a flag per
// launcher would skip the grant on the second device and fail at launch there.  One mutex covers the lookup and the ask: a pair is granted before any
// caller returns from it, and two threads never ask for the same thing twice.  A hit costs hipGetDevice and one find; only a first grant allocates.
static std::mutex g_lds_mutex;
static auto &g_lds_granted = *new std::map<std::pair<int, const void *>, size_t>;       // never destroyed: a thread may still launch while the process exits

int dl_lds_limit(const void *kern, size_t bytes, const char *who) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { dl_set_error("%s: hipGetDevice: %s", who, hipGetErrorString(e)); return -1; }
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    const auto it = g_lds_granted.find({dev, kern});
    if (it != g_lds_granted.end() && it->second >= bytes) return 0;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { dl_set_error("%s: hipFuncSetAttribute(%zu): %s", who, bytes, hipGetErrorString(e)); return -1; }
    if (it != g_lds_granted.end()) it->second = bytes;
    else g_lds_granted.emplace(std::make_pair(dev, kern), bytes);
    return 0;
}
extern "C" int dl_version(void) { return DL_VERSION; }

// ---- runtime switches: the variables below are copied out of the environment when the library is loaded; launches only read the copies
enum { DL_SW_LEN = 16 };
static const char *const g_sw_names[] = {"DL_CONV_S2F", "DL_CONV_S2FX3", "DL_CONV_W4X3", "DL_PACK_TILED", "DL_NO_X3_GLDS", "DL_NO_WGRAD_C4",          // (the order of switches.h)
                                         "DL_NO_C4_X3", "DL_CONV_S2D", "DL_CONV_DOT"};
static_assert(DL_SW_COUNT == sizeof(g_sw_names) / sizeof(*g_sw_names), "one name per switch id of switches.h");
static char g_sw_val[DL_SW_COUNT][DL_SW_LEN];
static bool g_sw_set[DL_SW_COUNT];

extern "C" void dl_switches_reload(void) {
    for (int i = 0; i < DL_SW_COUNT; ++i) {
        const char *v = getenv(g_sw_names[i]);
        g_sw_set[i] = v != nullptr;
        memset(g_sw_val[i], 0, DL_SW_LEN);          // (an unset variable leaves no stale value behind)
        if (v) strncpy(g_sw_val[i], v, DL_SW_LEN - 1);
    }
}
__attribute__((constructor)) static void dl_switches_init(void) { dl_switches_reload(); }

const char *dl_switch(int id) { return (id >= 0 && id < DL_SW_COUNT && g_sw_set[id]) ? g_sw_val[id] : nullptr; }

extern "C" int dl_switch_count(void) { return DL_SW_COUNT; }
extern "C" const char *dl_switch_name(int id) { return (id >= 0 && id < DL_SW_COUNT) ? g_sw_names[id] : nullptr; }
extern "C" int dl_half_format(void) {
#ifdef DL_H16_FP16
    return DL_HALF_FP16;
#else
    return DL_HALF_BF16;
#endif
}
extern "C" int dl_dev_build(void) {
#ifdef DL_DEV_SWITCHES
    return 1;
#else
    return 0;
#endif
}
