// lds_limit_check.cpp -- host run of dl_lds_limit (test infrastructure; built and run by tests/test_lds_limit_host.py, never linked into the library).
// error.cpp is compiled INTO this program with its two runtime calls renamed to the stand-ins below, so what runs is the library's own function and the
// library carries no test hook: a current device per thread as in HIP, a count of the asks, and a switch that makes the next ask fail.  Prints one line
// per case, "ok <case>" or "FAILED <case>: <what>", and exits with the number of failed cases.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdio.h>
#include <string.h>
#include <thread>
#include <vector>

static thread_local int t_device = 0;
static std::atomic<int> g_asks{0}, g_lookups{0}, g_last_value{0}, g_refuse_next{0};

static hipError_t check_get_device(int *dev) {
    ++g_lookups;
    *dev = t_device;
    return hipSuccess;
}
static hipError_t check_set_attribute(const void *, hipFuncAttribute attr, int value) {
    for (int i = 0; i < 16; ++i) std::this_thread::yield();          // (widens the window in which a second thread could ask for the same pair)
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
    ++g_asks;
    g_last_value = value;
    return g_refuse_next.exchange(0) ? hipErrorInvalidValue : hipSuccess;
}
#define hipGetDevice check_get_device
#define hipFuncSetAttribute check_set_attribute
#include "error.cpp"

static char g_kernels[512];          // distinct addresses stand for kernels; every case takes its own
static int g_failed = 0;
static void report(const char *name, bool ok, const char *what) {
    if (ok) printf("ok %s\n", name);
    else { printf("FAILED %s: %s\n", name, what); ++g_failed; }
}
// one call: the expected return value, the expected number of asks it makes, and exactly one look at the current device
static bool call(const void *k, size_t bytes, int want_ret, int want_asks) {
    const int asks = g_asks, lookups = g_lookups;
    return dl_lds_limit(k, bytes, "check") == want_ret && g_asks - asks == want_asks && g_lookups - lookups == 1;
}

int main() {
    const void *k = &g_kernels[0];
    t_device = 0;
    report("asks_once", call(k, 70000, 0, 1) && g_last_value == 70000 && call(k, 70000, 0, 0) && call(k, 70000, 0, 0), "first call or repeat");

    // the case a process-wide flag gets wrong: the same kernel on another device
    t_device = 1;
    bool ok = call(k, 70000, 0, 1) && call(k, 70000, 0, 0);
    t_device = 0;
    report("second_device_asks_again", ok && call(k, 70000, 0, 0), "device 1 after device 0, or device 0 again");

    k = &g_kernels[1];
    report("larger_asks_smaller_does_not", call(k, 70000, 0, 1) && call(k, 90000, 0, 1) && g_last_value == 90000 && call(k, 80000, 0, 0) && call(k, 90000, 0, 0) &&
                                               call(k, 90001, 0, 1), "sizes 70000, 90000, 80000, 90000, 90001");

    k = &g_kernels[2];
    g_refuse_next = 1;
    ok = dl_lds_limit(k, 70000, "check(refused)") == -1 && g_refuse_next == 0;
    const char *want = "check(refused): hipFuncSetAttribute(70000): ";
    ok = ok && strncmp(dl_last_error(), want, strlen(want)) == 0 && strlen(dl_last_error()) > strlen(want);
    report("refusal_is_reported_and_retried", ok && call(k, 70000, 0, 1) && call(k, 70000, 0, 0), dl_last_error());
    // a refused increase leaves the earlier grant standing
    g_refuse_next = 1;
    report("refused_increase_keeps_the_grant", call(k, 90000, -1, 1) && call(k, 70000, 0, 0) && call(k, 90000, 0, 1) && call(k, 90000, 0, 0), "70000 granted, 90000 refused once");

    ok = true;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < 200; ++i) ok = ok && call(&g_kernels[100 + i], 70000, 0, pass == 0 ? 1 : 0);
    report("200_kernels_stay_remembered", ok, "a kernel asked twice, or not at all");

    // eight threads over 2 devices x 4 kernels, all started together: 8 asks in all, every call succeeds
    const int asks = g_asks;
    std::atomic<int> ready{0}, bad{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < 8; ++t)
        threads.emplace_back([&, t] {
            ++ready;
            while (ready < 8) std::this_thread::yield();
            for (int i = 0; i < 400; ++i) {
                const int j = (i + t) % 8;
                t_device = j >> 2;
                if (dl_lds_limit(&g_kernels[400 + (j & 3)], 70000, "check(threads)") != 0) ++bad;
            }
        });
    for (auto &th : threads) th.join();
    report("eight_threads_ask_eight_times", bad == 0 && g_asks - asks == 8, "more or fewer than 8 asks, or a failed call");
    return g_failed;
}
