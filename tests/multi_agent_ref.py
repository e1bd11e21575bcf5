"""float64 numpy references of the multi-agent path (one agent per turbine, one shared policy), kept with the tests."""
import numpy as np


def gae_shared(reward, value, final_value, truncated, gamma, lam):
    """Shared-reward GAE: reward / truncated [T, B] belong to the env, value / final_value [T, B, A] to its agents.
    delta[t, b, a] = reward[t, b] + gamma final_value[t, b, a] - value[t, b, a],
    A[t, b, a] = delta[t, b, a] + gamma lam (1 - truncated[t, b]) A[t + 1, b, a], A[T] = 0, returns = A + value."""
    r = np.asarray(reward, np.float64)
    v, fv = np.asarray(value, np.float64), np.asarray(final_value, np.float64)
    cont = 1.0 - np.asarray(truncated).astype(np.float64)
    T, B, A = v.shape
    assert r.shape == (T, B) and cont.shape == (T, B) and fv.shape == (T, B, A)
    adv = np.zeros_like(v)
    a = np.zeros((B, A))
    for t in range(T - 1, -1, -1):
        a = r[t][:, None] + gamma * fv[t] - v[t] + gamma * lam * cont[t][:, None] * a
        adv[t] = a
    return adv, adv + v


def gae_shared_brute(reward, value, final_value, truncated, gamma, lam):
    """The same by definition, one agent row at a time: the discounted sum of the row's deltas up to and including the env's
    first truncation at or after t (or the end of the buffer)."""
    r = np.asarray(reward, np.float64)
    v, fv = np.asarray(value, np.float64), np.asarray(final_value, np.float64)
    tr = np.asarray(truncated).astype(bool)
    T, B, A = v.shape
    adv = np.zeros((T, B, A))
    for b in range(B):
        for a in range(A):
            for t in range(T):
                s, w, acc = t, 1.0, 0.0
                while s < T:
                    acc += w * (r[s, b] + gamma * fv[s, b, a] - v[s, b, a])
                    if tr[s, b]:
                        break
                    w *= gamma * lam
                    s += 1
                adv[t, b, a] = acc
    return adv, adv + v
