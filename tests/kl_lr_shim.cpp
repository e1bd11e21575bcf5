// kl_lr_shim.cpp — hands the KL-adaptive learning-rate rule of windgym_amd/csrc/wg_train.h (the function the Adam kernels call) to
// tests/test_kl_lr_host.py.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/kl_lr_shim.cpp
#include <string.h>

#include "wg_train.h"

// the public arguments -> out[6] = kl_low, kl_high, up, down, lr_min, lr_max
extern "C" void kl_lr_rule(float desired_kl, float factor, float lr_min, float lr_max, float* out) {
    const WgKlLr r = wg_kl_lr_rule(desired_kl, factor, lr_min, lr_max);
    const float v[6] = {r.kl_low, r.kl_high, r.up, r.down, r.lr_min, r.lr_max};
    memcpy(out, v, sizeof(v));
}

// one step of the rule `r[6]` (the order above)
extern "C" float kl_lr_next(float lr, float kl, const float* r) {
    const WgKlLr rule = {r[0], r[1], r[2], r[3], r[4], r[5]};
    return wg_kl_lr_next(lr, kl, rule);
}

// what is wrong with the public arguments ("" : nothing)
extern "C" const char* kl_lr_refusal(float desired_kl, float factor, float lr_min, float lr_max) {
    const char* s = wg_kl_lr_refusal(desired_kl, factor, lr_min, lr_max);
    return s ? s : "";
}

// the words of minibatch mb as offsets: 0 = the caller's word, 1 / 2 = the two slots, -1 = none; out[0] = read, out[1] = written
extern "C" void kl_lr_words(int mb, int last, int* out) {
    static float word[1], slots[2];
    const float* in;
    float* to;
    wg_kl_lr_words(word, slots, mb, last, &in, &to);
    out[0] = in == word ? 0 : (int)(in - slots) + 1;
    out[1] = !to ? -1 : to == word ? 0 : (int)(to - slots) + 1;
}

// the host's half of Adam's scalars with the rate on the device: out[0] = bc1 (double), -> bc2_sqrt
extern "C" float adam_kl_scalars(uint64_t step, double* bc1) {
    const WgAdamKlStep s = wg_adam_kl_scalars(step);
    *bc1 = s.bc1;
    return s.bc2_sqrt;
}

extern "C" void adam_scalars(uint64_t step, float lr, float* out) {
    const WgAdamStep s = wg_adam_scalars(step, lr);
    out[0] = s.step_size; out[1] = s.bc2_sqrt;
}
