// wg_devmem.h — the owner of a handle's device memory as the handle structs hold it.  Plain C++ (wg_policy.h, wg_ppo.h and wg_lstm.h
// are read by g++ alone in the tests); the member functions are defined in wg_host.h, which states their rules.
#pragma once
#include <stddef.h>

#include <vector>

struct WgDevMem {
    int device = 0;
    std::vector<void*> ptrs;          // every live allocation, in the order it was made
    int alloc_bytes(const char* who, void** out, size_t bytes, bool zero);
    template <class T>
    int alloc(const char* who, T** out, size_t n, bool zero = true) { return alloc_bytes(who, (void**)out, sizeof(T) * (n ? n : 1), zero); }
    int free(const char* who, void* ptr);
    void release();
};
