// wg_host.h — what every host function of the library starts with: report an error through the thread-local message behind
// wg_last_error, check a HIP call, make a handle's device the current one.  (include after <hip/hip_runtime.h>; wg_mann.hip's
// goto-style check is a different shape and stays its own)
#pragma once
#include <string>

#include "wg_internal.h"

static inline int wg_fail(int code, const std::string& msg) { return wg_set_last_error_(code, msg.c_str()); }

#define WG_HIPCHK(x)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (x);                                                                              \
        if (_e != hipSuccess) return wg_fail(WG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
    } while (0)

// What makes handles a population, refused once for wg_pop_* and wg_lstm_pop_* (`who`: the entry, or "entry: member m")
static inline int wg_pop_count(const char* who, int P) {
    if (P >= 1 && P <= WG_POP_MAX) return 0;
    return wg_fail(WG_ERR_INVALID, std::string(who) + ": a population has 1 .. " + std::to_string(WG_POP_MAX) + " members, not " + std::to_string(P));
}

// the members own equal shares of n rows `of` what; the count is spelled `before` n `after` ("7 rows do", "B = 7 does")
static inline int wg_pop_shares(const std::string& who, int P, long long n, const char* of, const char* before, const char* after) {
    if (n % P == 0) return 0;
    const std::string p = std::to_string(P);
    return wg_fail(WG_ERR_INVALID, who + ": the " + p + " members own equal shares of the " + of + ", and " + before + std::to_string(n) + after + " not divide by " + p);
}

// member m brings no handle an earlier member k brought; `says` ends the message in front of k
template <class... H>
static inline int wg_pop_given_twice(const std::string& who, int m, const char* says, const H*... handles) {
    for (int k = 0; k < m; ++k)
        if (((handles[k] == handles[m]) || ...)) return wg_fail(WG_ERR_INVALID, who + says + std::to_string(k));
    return 0;
}

// member m's handles live on member 0's device dev0; `what` names them where a member has more than one
template <class... D>
static inline int wg_pop_same_device(const std::string& who, int dev0, const char* what, D... dev) {
    if (((dev == dev0) && ...)) return 0;
    std::string on;
    ((on += (on.empty() ? "" : " / ") + std::to_string(dev)), ...);
    return wg_fail(WG_ERR_INVALID, who + " lives on device " + on + what + ", member 0 on device " + std::to_string(dev0));
}

// what both population updates refuse alike (`epochs`: what must be >= 1, as the entry words it)
static inline int wg_pop_update_check(const char* who, bool has_opts, bool counts_ok, const char* epochs, int P, float* const* params_dev,
                                      const float* max_grad_norm) {
    const std::string w = who;
    if (!has_opts) return wg_fail(WG_ERR_INVALID, w + ": the population was created without optimisers (opts = NULL): it only acts");
    if (!counts_ok) return wg_fail(WG_ERR_INVALID, w + ": " + epochs + " must be >= 1");
    for (int m = 0; m < P; ++m) {
        if (!params_dev[m]) return wg_fail(WG_ERR_INVALID, w + ": member " + std::to_string(m) + ": params_dev is null");
        if (!(max_grad_norm[m] > 0.0f)) return wg_fail(WG_ERR_INVALID, w + ": member " + std::to_string(m) + ": max_grad_norm must be > 0");
    }
    return 0;
}

static inline int wg_use_device(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) {
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    }
    return 0;
}
