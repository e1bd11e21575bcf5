// train_shim.cpp — hands windgym_amd/csrc/wg_train.h (Adam's per-step scalars, the minibatch loop) to tests/test_train_host.py.
// Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/train_shim.cpp
#include "wg_train.h"

extern "C" void adam_consts(double* out) { out[0] = ADAM_B1; out[1] = ADAM_B2; out[2] = ADAM_EPS; }

extern "C" void adam_scalars(uint64_t step, float lr, float* out) {
    const WgAdamStep s = wg_adam_scalars(step, lr);
    out[0] = s.step_size; out[1] = s.bc2_sqrt;
}

// two steps counted on one WgAdam from `step`: out = the scalars of step + 1 and of step + 2; -> the count afterwards
extern "C" uint64_t adam_count_twice(uint64_t step, float lr, float* out) {
    WgAdam a = {};
    a.step = step;
    for (int i = 0; i < 2; ++i) {
        const WgAdamStep s = wg_adam_count(&a, lr);
        out[2 * i] = s.step_size; out[2 * i + 1] = s.bc2_sqrt;
    }
    return a.step;
}

extern "C" int n_minibatches(int64_t rows, int batch) { return wg_n_minibatches(rows, batch); }

// the walk as (mb, off, n) triples into out[3 * cap]; stop_at >= 0: f returns 7 at that call -> the walk's return value in *rc
extern "C" int each_minibatch(int64_t rows, int n_epochs, int batch, int stop_at, int64_t* out, int cap, int* rc) {
    int calls = 0;
    *rc = wg_each_minibatch(rows, n_epochs, batch, [&](int mb, int64_t off, int n) {
        if (calls < cap) { out[3 * calls] = mb; out[3 * calls + 1] = off; out[3 * calls + 2] = n; }
        return calls++ == stop_at ? 7 : 0;
    });
    return calls;
}
