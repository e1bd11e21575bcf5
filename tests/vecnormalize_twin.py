"""Test-only float64 numpy restatement of stable-baselines3 2.x's ``RunningMeanStd`` (common/running_mean_std.py) and ``VecNormalize``
(common/vec_env/vec_normalize.py) as include/windgym_hip.h pins them: the reference of test_vecnormalize.py and
test_gpu_vecnormalize.py.  SB3 itself is not a dependency; test_vecnormalize.py checks this restatement by hand-computed values."""
import numpy as np


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, np.float64), np.ones(shape, np.float64), 1e-4

    def update(self, batch):
        batch = np.asarray(batch, np.float64)
        n = batch.shape[0]
        bm = batch.mean(axis=0)
        bv = ((batch - bm) ** 2).mean(axis=0)                 # the population variance about bm
        delta = bm - self.mean
        tot = self.count + n
        mean = self.mean + delta * n / tot
        m2 = self.var * self.count + bv * n + np.square(delta) * self.count * n / tot
        self.mean, self.var, self.count = mean, m2 / tot, tot


class VecNormalizeTwin:
    """The wrapper's rules on arrays the caller supplies (there is no env in here): ``reset(obs)``, ``step(obs, reward, done,
    final_obs)`` -> what the wrapper returns.  Outputs are float64 values rounded to float32 once."""

    def __init__(self, n_obs, n_envs, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8):
        self.obs_rms, self.ret_rms = RunningMeanStd((n_obs,)), RunningMeanStd(())
        self.returns = np.zeros(n_envs, np.float64)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)

    def normalize_obs(self, x):
        if not self.norm_obs:
            return np.asarray(x, np.float32)
        x = np.asarray(x, np.float64)
        return np.clip((x - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_reward(self, r):
        if not self.norm_reward:
            return np.asarray(r, np.float32)
        r = np.asarray(r, np.float64)
        return np.clip(r / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward).astype(np.float32)

    def reset(self, obs):
        self.returns[:] = 0.0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def obs_half(self, obs, final_obs=None):
        """Rules 2, 3 and 6: -> (normalised obs, normalised final rows or None)"""
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs), None if final_obs is None else self.normalize_obs(final_obs)

    def reward_half(self, reward, done):
        """Rules 4, 5 and 7 for one step"""
        if self.training:
            self.returns = self.returns * self.gamma + np.asarray(reward, np.float64)
            self.ret_rms.update(self.returns)
        r_n = self.normalize_reward(reward)
        self.returns[np.asarray(done).astype(bool)] = 0.0
        return r_n

    def step(self, obs, reward, done, final_obs=None):
        obs_n, fin_n = self.obs_half(obs, final_obs)
        return obs_n, self.reward_half(reward, done), fin_n

    def reward_pass(self, reward, done):
        """``reward_half`` over ``[T, B]``"""
        return np.stack([self.reward_half(r, d) for r, d in zip(reward, done)])
