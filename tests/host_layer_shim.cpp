// host_layer_shim.cpp — hands the host layer of windgym_amd/csrc/wg_host.h (the owner of device memory, the pointer check, the blob
// frame) to tests/test_host_layer.py on a SCRIPTED FAKE DEVICE: stand-ins for the few HIP names the header uses come first, then
// the header itself.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/host_layer_shim.cpp
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

// ---- the stand-ins ----------------------------------------------------------------------------------------------------------------
typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorInvalidDevice = 101 };
enum hipMemoryType { hipMemoryTypeHost = 1, hipMemoryTypeDevice = 2 };
struct hipPointerAttribute_t { hipMemoryType type; int device; };

namespace fake {
enum Op { MALLOC, MEMSET, SETDEVICE, N_OPS };
enum Event { SYNC = 1, FREE = 2, COPY = 3 };
struct Ptr { int device; hipMemoryType type; };
int current = 0;
int calls[N_OPS], fail_at[N_OPS], fail_err[N_OPS];        // the k-th call (from 0) of an op fails with fail_err; -1: none
std::map<void*, Ptr> live;
std::map<void*, int> frees;
std::vector<int> events, sync_device;
std::vector<size_t> malloc_bytes;               // what every successful hipMalloc was asked for
uintptr_t next_address = 0x10000;
std::string last_error;

void reset() {
    current = 0;
    for (int o = 0; o < N_OPS; ++o) { calls[o] = 0; fail_at[o] = -1; fail_err[o] = 0; }
    live.clear(); frees.clear(); events.clear(); sync_device.clear(); malloc_bytes.clear(); last_error.clear();
}
hipError_t scripted(Op o) { return calls[o]++ == fail_at[o] ? fail_err[o] : hipSuccess; }
}  // namespace fake

static hipError_t hipGetDevice(int* d) { *d = fake::current; return hipSuccess; }
static hipError_t hipSetDevice(int d) {
    if (hipError_t e = fake::scripted(fake::SETDEVICE)) return e;
    fake::current = d;
    return hipSuccess;
}
static hipError_t hipMalloc(void** out, size_t bytes) {
    if (hipError_t e = fake::scripted(fake::MALLOC)) return e;
    *out = (void*)(fake::next_address += 0x100);           // never dereferenced, never handed out twice
    fake::live[*out] = {fake::current, hipMemoryTypeDevice};
    fake::malloc_bytes.push_back(bytes);
    return hipSuccess;
}
static hipError_t hipMemset(void*, int, size_t) { return fake::scripted(fake::MEMSET); }
static hipError_t hipFree(void* p) {
    fake::events.push_back(fake::FREE);
    ++fake::frees[p];
    fake::live.erase(p);
    return hipSuccess;
}
static hipError_t hipDeviceSynchronize() {
    fake::events.push_back(fake::SYNC);
    fake::sync_device.push_back(fake::current);
    return hipSuccess;
}
static hipError_t hipGetLastError() { return hipSuccess; }
static const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorInvalidDevice ? "invalid device ordinal" : "invalid argument";
}
static hipError_t hipPointerGetAttributes(hipPointerAttribute_t* at, const void* p) {
    const auto it = fake::live.find(const_cast<void*>(p));
    if (it == fake::live.end()) return hipErrorInvalidValue;
    at->type = it->second.type; at->device = it->second.device;
    return hipSuccess;
}

// ---- the header under test --------------------------------------------------------------------------------------------------------
#include "wg_host.h"

extern "C" int wg_set_last_error_(int code, const char* msg) {
    fake::last_error = msg ? msg : "";
    return code;
}

// ---- what the tests call ----------------------------------------------------------------------------------------------------------
extern "C" {
void fake_reset() { fake::reset(); }
void fake_fail(int op, int k, int err) { fake::fail_at[op] = k; fake::fail_err[op] = err; }
void fake_set_current(int d) { fake::current = d; }
int fake_current() { return fake::current; }
// memory the owner did not allocate: of `device`, host-typed (type 1) or device-typed (2)
void* fake_foreign(int device, int type) {
    void* p = (void*)(fake::next_address += 0x100);
    fake::live[p] = {device, (hipMemoryType)type};
    return p;
}
int fake_n_live() { return (int)fake::live.size(); }
int fake_frees_of(void* p) { const auto it = fake::frees.find(p); return it == fake::frees.end() ? 0 : it->second; }
int fake_n_frees() { int n = 0; for (const auto& f : fake::frees) n += f.second; return n; }
int fake_most_frees() { int n = 0; for (const auto& f : fake::frees) n = f.second > n ? f.second : n; return n; }
size_t fake_malloc_bytes(int i) { return fake::malloc_bytes[i]; }
int fake_n_sync() { return (int)fake::sync_device.size(); }
int fake_sync_device(int i) { return fake::sync_device[i]; }
int fake_events(int* out, int cap) {
    for (int i = 0; i < (int)fake::events.size() && i < cap; ++i) out[i] = fake::events[i];
    return (int)fake::events.size();
}
const char* last_error() { return fake::last_error.c_str(); }
int err_codes(int which) { return which == 0 ? WG_ERR_INVALID : which == 1 ? WG_ERR_HIP : WG_ERR_NOMEM; }

WgDevMem* owner_new(int device) { WgDevMem* m = new WgDevMem; m->device = device; return m; }
void owner_delete(WgDevMem* m) { delete m; }
int owner_alloc(WgDevMem* m, const char* who, size_t n, int zero, float** out) { return m->alloc(who, out, n, zero != 0); }
int owner_free(WgDevMem* m, const char* who, void* p) { return m->free(who, p); }
void owner_release(WgDevMem* m) { m->release(); }
int owner_held(const WgDevMem* m) { return (int)m->ptrs.size(); }

int on_device(const char* prefix, int device, const void* ptr, const char* name, const char* whose) {
    return wg_on_device(prefix, device, ptr, name, whose);
}
// the table form on three entries
int on_device_all(const char* who, const char* prefix, int device, const void* const* ptr, const char* const* name, const int* required,
                  const char* whose) {
    const WgPtrArg args[3] = {{ptr[0], name[0], required[0] != 0}, {ptr[1], name[1], required[1] != 0}, {ptr[2], name[2], required[2] != 0}};
    return wg_on_device_all(who, prefix, device, args, whose);
}

// a handle's blob: this header, then `payload` bytes
struct ShimHeader { uint32_t magic; int32_t rows, cols, reserved; };
const uint32_t SHIM_MAGIC = 0x4d494853u;
size_t blob_header_bytes() { return sizeof(ShimHeader); }
uint32_t blob_magic() { return SHIM_MAGIC; }
int blob_get(const char* prefix, int device, void* host, size_t* size, size_t total) {
    if (int rc = wg_blob_get(prefix, device, host, size, total)) return rc;
    if (!host) return 0;
    fake::events.push_back(fake::COPY);
    return 0;
}
int blob_set(const char* prefix, int device, const void* host, size_t size, const char* not_ours, int rows, int cols) {
    const auto geometry = [&](const ShimHeader& got) {
        if (got.rows == rows && got.cols == cols) return 0;
        return wg_fail(WG_ERR_INVALID, "shim: the blob is " + std::to_string(got.rows) + " x " + std::to_string(got.cols));
    };
    if (int rc = wg_blob_set<ShimHeader>(prefix, device, host, size, SHIM_MAGIC, not_ours, geometry)) return rc;
    fake::events.push_back(fake::COPY);
    return 0;
}
}
