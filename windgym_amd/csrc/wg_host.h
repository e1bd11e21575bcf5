// wg_host.h — what every host function of the library starts with, stated once: report an error through the thread-local message
// behind wg_last_error (wg_fail), check a HIP call (WG_HIPCHK), make a handle's device the current one (wg_use_device), own a
// handle's device memory (WgDevMem), check that a caller's pointer is memory of the handle's device (wg_on_device, wg_on_device_all),
// frame a state blob (wg_blob_get, wg_blob_set), and what makes handles a population (wg_pop_*).  It includes no HIP header: include
// it after <hip/hip_runtime.h> — tests/host_layer_shim.cpp puts a scripted fake device there instead.  (wg_mann.hip's goto-style
// check is a different shape and stays its own)
#pragma once
#include <string.h>

#include <algorithm>
#include <string>

#include "wg_devmem.h"
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

// ---- the owner of a handle's device memory (wg_devmem.h: WgDevMem) ---------------------------------------------------------------
// THE RULE FOR A FAILING HIP CALL: it is reported as `who`, WG_ERR_NOMEM when the device is out of memory and WG_ERR_HIP otherwise;
// the owner keeps everything it allocated before, and the handle's ordinary destroy — one release() — frees it.  release() makes
// the device current, synchronises it once and frees every pointer exactly once; where the device cannot be made current it skips
// the synchronisation and frees all the same (a leak helps nobody).  It leaves the owner empty: a second release() does nothing.
static inline int wg_hip_fail(const char* who, hipError_t e) {
    return wg_fail(e == hipErrorOutOfMemory ? WG_ERR_NOMEM : WG_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// `bytes` on the owner's device, which becomes the current one; an allocation whose hipMemset fails is given back at once
inline int WgDevMem::alloc_bytes(const char* who, void** out, size_t bytes, bool zero) {
    if (int rc = wg_use_device(device)) return rc;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && zero && (e = hipMemset(p, 0, bytes)) != hipSuccess) (void)hipFree(p);
    if (e != hipSuccess) return wg_hip_fail(who, e);
    ptrs.push_back(p);
    *out = p;
    return 0;
}

// one buffer that is replaced during the handle's life (null, or not the owner's: nothing happens); the caller has made the device
// current and idle
inline int WgDevMem::free(const char* who, void* ptr) {
    const auto it = std::find(ptrs.begin(), ptrs.end(), ptr);
    if (!ptr || it == ptrs.end()) return 0;
    ptrs.erase(it);
    const hipError_t e = hipFree(ptr);
    return e == hipSuccess ? 0 : wg_hip_fail(who, e);
}

inline void WgDevMem::release() {
    if (ptrs.empty()) return;
    if (wg_use_device(device) == 0) (void)hipDeviceSynchronize();
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
}

// ---- a buffer a kernel will touch must be device memory of the handle's device ---------------------------------------------------
// `prefix` opens the message in front of the argument's `name`; `whose` closes the wrong-device form (", the table's device"; "")
static inline int wg_on_device(const std::string& prefix, int device, const void* ptr, const char* name, const char* whose) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return wg_fail(WG_ERR_INVALID, prefix + name + " is not a device pointer");
    }
    if (at.type != hipMemoryTypeDevice || at.device != device)
        return wg_fail(WG_ERR_INVALID, prefix + name + " is not memory of device " + std::to_string(device) + whose);
    return 0;
}

// an entry's pointer arguments in order, the first bad one reported: a null one as `who` NAME is null when it is required (skipped
// when it is not), the others as wg_on_device words it
struct WgPtrArg { const void* ptr; const char* name; bool required; };
template <size_t N>
static inline int wg_on_device_all(const std::string& who, const std::string& prefix, int device, const WgPtrArg (&args)[N], const char* whose) {
    for (const WgPtrArg& a : args) {
        if (!a.ptr) {
            if (a.required) return wg_fail(WG_ERR_INVALID, who + a.name + " is null");
            continue;
        }
        if (int rc = wg_on_device(prefix, device, a.ptr, a.name, whose)) return rc;
    }
    return 0;
}

// ---- the frame of a state blob: a header struct H that starts with its uint32_t magic, then the handle's payload ------------------
// get_state: the size query (host == NULL: *size = total and nothing else; the caller returns 0 then), the room, and the device
// current and idle for the caller's copies.  `prefix` opens the messages ("" for wg_get_state)
static inline int wg_blob_get(const char* prefix, int device, const void* host, size_t* size, size_t total) {
    if (!host) {
        *size = total;
        return 0;
    }
    if (*size < total) return wg_fail(WG_ERR_INVALID, std::string(prefix) + "state buffer too small");
    if (int rc = wg_use_device(device)) return rc;
    WG_HIPCHK(hipDeviceSynchronize());
    return 0;
}

// set_state: the blob holds a header, the header is the handle's kind (`not_ours`: the handle's own words for another magic) and
// `geometry(got)`, the caller's comparison with its own words, passes; then the device is current and idle for the caller's copies
template <class H, class G>
static inline int wg_blob_set(const char* prefix, int device, const void* host, size_t size, uint32_t magic, const char* not_ours, G geometry) {
    if (size < sizeof(H)) return wg_fail(WG_ERR_INVALID, std::string(prefix) + "state blob too small");
    H got;
    memcpy(&got, host, sizeof(got));
    if (got.magic != magic) return wg_fail(WG_ERR_INVALID, std::string(prefix) + not_ours);
    if (int rc = geometry(got)) return rc;
    if (int rc = wg_use_device(device)) return rc;
    WG_HIPCHK(hipDeviceSynchronize());
    return 0;
}

// ---- populations -----------------------------------------------------------------------------------------------------------------
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
