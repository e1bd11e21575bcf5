// wg_train.h — what the trainers' host code shares and a plain C++ compiler can read (no HIP include: tests/train_shim.cpp hands it to
// tests/test_train_host.py): Adam's constants, its per-step scalars, its state object, and the minibatch loop of one update.
// The functions on a WgAdam that touch the device are wg_adam_*_ of wg_internal.h (wg_ppo.hip).
#pragma once
#include <stdint.h>

#include <cmath>

// Adam's constants (the kernels take 1 - beta1, beta2, 1 - beta2 and eps)
static const double ADAM_B1 = 0.9, ADAM_B2 = 0.999;
static const float ADAM_EPS = 1e-5f;

struct WgAdamStep { float step_size, bc2_sqrt; };        // lr / (1 - beta1^step), sqrt(1 - beta2^step)

// the scalars of step number `step` >= 1 (bias corrections in double, rounded once)
static inline WgAdamStep wg_adam_scalars(uint64_t step, float lr) {
    const double bc1 = 1.0 - std::pow(ADAM_B1, (double)step), bc2 = 1.0 - std::pow(ADAM_B2, (double)step);
    return {(float)((double)lr / bc1), (float)std::sqrt(bc2)};
}

// Adam over one flat vector of n_flat parameters on `device`
struct WgAdam {
    int device;
    uint32_t n_flat, n_blocks;            // n_blocks = ceil(n_flat / WGT_BLOCK)
    uint64_t step;                        // steps taken
    float *m, *v, *blocksq;               // [n_flat] the moments; [n_blocks] partial sums of squares of the gradient
};

// counts one more step of `a` and -> that step's scalars
static inline WgAdamStep wg_adam_count(WgAdam* a, float lr) { return wg_adam_scalars(++a->step, lr); }

// One update: n_epochs passes over `rows` rows (one row of the permutation each) in minibatches of batch_size, the last one of
// an epoch shorter.  f(mb, off, n) runs once per minibatch, in order: mb = its index in the update (the slot of its
// statistics), off = its offset into the permutation, n = its rows.  A non-zero return of f ends the walk and is returned.
static inline int wg_n_minibatches(int64_t rows, int batch_size) { return (int)((rows + batch_size - 1) / batch_size); }
template <class F>
static inline int wg_each_minibatch(int64_t rows, int n_epochs, int batch_size, F f) {
    const int n_mb = wg_n_minibatches(rows, batch_size);
    for (int e = 0; e < n_epochs; ++e)
        for (int k = 0; k < n_mb; ++k) {
            const int64_t start = (int64_t)k * batch_size;
            const int n = (int)(rows - start < batch_size ? rows - start : batch_size);
            if (int rc = f(e * n_mb + k, (int64_t)e * rows + start, n)) return rc;
        }
    return 0;
}
