// wg_train.h — what the trainers' host code shares and a plain C++ compiler can read (no HIP include: tests/train_shim.cpp hands it to
// tests/test_train_host.py): Adam's constants, its per-step scalars, its state object, the KL-adaptive learning-rate rule (which
// the Adam kernels read too: tests/kl_lr_shim.cpp), and the minibatch loop of one update.
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

// ... and with the rate in device memory: the host's half, 1 - beta1^step in double; the kernel then forms step_size by the
// expression above from the rate it read (an IEEE double division on both sides: the same bits)
struct WgAdamKlStep { double bc1; float bc2_sqrt; };
static inline WgAdamKlStep wg_adam_kl_scalars(uint64_t step) {
    return {1.0 - std::pow(ADAM_B1, (double)step), wg_adam_scalars(step, 0.0f).bc2_sqrt};
}

// ---- the KL-adaptive learning rate (windgym_hip.h: wg_ppo_set_kl_lr), host and device from ONE statement --------------------------
#ifdef __HIPCC__
#define WG_HD __host__ __device__
#else
#define WG_HD
#endif

// the rule as the kernels hold it: the band kl_low < kl < kl_high in which the rate stays, the two factors and the clamp
struct WgKlLr { float kl_low, kl_high, up, down, lr_min, lr_max; };

// the rate of the next optimiser step from the one before and the minibatch's approx_kl.  Multiplications only: `down` is 1 / factor
// rounded once on the host, so host and device agree to the bit.  Inside the band, kl == 0, kl < 0, NaN: unchanged
WG_HD static inline float wg_kl_lr_next(float lr, float kl, const WgKlLr& r) {
    if (kl > r.kl_high) return fmaxf(r.lr_min, lr * r.down);
    if (kl < r.kl_low && kl > 0.0f) return fminf(r.lr_max, lr * r.up);
    return lr;
}

// the public arguments -> the rule: rsl_rl's band desired_kl / 2 .. 2 desired_kl, in float
static inline WgKlLr wg_kl_lr_rule(float desired_kl, float factor, float lr_min, float lr_max) {
    return {desired_kl / 2.0f, 2.0f * desired_kl, factor, 1.0f / factor, lr_min, lr_max};
}

// what is wrong with the public arguments, naming the argument, or null
static inline const char* wg_kl_lr_refusal(float desired_kl, float factor, float lr_min, float lr_max) {
    if (!(desired_kl > 0.0f) || !std::isfinite(desired_kl)) return "desired_kl must be > 0 and finite";
    if (!(factor >= 1.0f) || !std::isfinite(factor)) return "factor must be >= 1 and finite";
    if (!(lr_min > 0.0f)) return "lr_min must be > 0";
    if (!(lr_min <= lr_max)) return "lr_min must be <= lr_max";
    return nullptr;
}

// The words minibatch mb (0 .. of an update, `last`: its final one) reads its rate from and writes the rate it used to.  The rate
// travels from the caller's word lr_dev through two slots alternated by the minibatch's parity back to lr_dev, so that in -> out are
// never one word: every block of the Adam kernel recomputes the rate from *in while one thread writes *out.  The first minibatch
// leaves the rate as it is (out = null when it is also the last: lr_dev already holds it).
WG_HD static inline void wg_kl_lr_words(float* lr_dev, float* slots, int mb, int last, const float** in, float** out) {
    *in = mb == 0 ? lr_dev : slots + ((mb - 1) & 1);
    *out = last ? (mb == 0 ? nullptr : lr_dev) : slots + (mb & 1);
}

// Adam over one flat vector of n_flat parameters on `device`
struct WgAdam {
    int device;
    uint32_t n_flat, n_blocks;            // n_blocks = ceil(n_flat / WGT_BLOCK)
    uint64_t step;                        // steps taken
    float *m, *v, *blocksq;               // [n_flat] the moments; [n_blocks] partial sums of squares of the gradient
    float* lr_slots;                      // [2] the KL-adaptive rate on its way through an update (wg_kl_lr_words); null until a rule is set
    float* lr_dev;                        // the caller's rate word while a KL rule is set, else null
    WgKlLr rule;
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
