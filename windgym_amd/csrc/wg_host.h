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

static inline int wg_use_device(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) {
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    }
    return 0;
}
