"""The rollout bookkeeping's contract (include/microrts_amd.h) in numpy: what k_episode_update and
k_gae (csrc/mrts_rollout.hip) must equal bit for bit.  Also the advantage loop as the reference
writes it in torch (python-float scalars times float32 tensors), for either device, and the bound
of the host wrappers' float32 discount against the contract's float64 one."""
import numpy as np

ROW = 18   # env, step, r, l, rawsum[6], disc[7], 0


class EpisodeStatsRef:
    """The update of include/microrts_amd.h: every operation one numpy operation of the stated
    type (numpy never fuses).  State arrays as the device buffer holds them; `ring` [capacity, ROW];
    `count` records since creation; `steps` calls so far."""

    def __init__(self, num_envs, gamma=0.99, capacity=None):
        self.n, self.gamma = int(num_envs), float(gamma)
        self.capacity = max(4 * self.n, 1024) if capacity is None else int(capacity)
        self.ret = np.zeros(self.n, np.float32)
        self.len = np.zeros(self.n, np.int32)
        self.factor = np.ones(self.n, np.float64)
        self.rawsum = np.zeros((6, self.n), np.float64)
        self.disc = np.zeros((7, self.n), np.float64)
        self.ring = np.zeros((self.capacity, ROW), np.float64)
        self.count = self.steps = 0
        self.records = []   # every record ever written, in order (the ring forgets)

    def update(self, reward, done, raw):
        reward, raw = np.asarray(reward, np.float64), np.asarray(raw, np.float64)
        done = np.asarray(done).astype(bool)
        assert reward.shape == (self.n,) and done.shape == (self.n,) and raw.shape == (self.n, 6)
        self.ret = (self.ret.astype(np.float64) + reward).astype(np.float32)
        self.len = self.len + np.int32(1)
        x = raw.T
        for k in range(6):
            self.rawsum[k] = self.rawsum[k] + x[k]
        tot = ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]
        for k in range(6):
            self.disc[k] = self.disc[k] + self.factor * x[k]
        self.disc[6] = self.disc[6] + self.factor * tot
        self.factor = self.factor * self.gamma
        ended = np.flatnonzero(done)
        for j, e in enumerate(ended):
            row = np.concatenate(([e, self.steps, np.float64(self.ret[e]), self.len[e]], self.rawsum[:, e], self.disc[:, e], [0.0]))
            self.records.append(row)
            if j >= len(ended) - self.capacity:   # a call that ends more than the ring holds keeps its last ones
                self.ring[(self.count + j) % self.capacity] = row
        self.count += len(ended)
        self.ret[ended], self.len[ended], self.factor[ended] = 0, 0, 1
        self.rawsum[:, ended] = 0
        self.disc[:, ended] = 0
        self.steps += 1


def gae_ref(rewards, values, dones, last_value, last_done, gamma=0.99, gae_lambda=0.95, use_gae=True):
    """Both modes in float32, each operation rounded on its own; dones of any dtype are read as float32."""
    f = np.float32
    r, v = np.asarray(rewards, f), np.asarray(values, f)
    d, ld, lv = np.asarray(dones).astype(f), np.asarray(last_done).astype(f), np.asarray(last_value, f)
    T = r.shape[0]
    g, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    adv, ret = np.zeros_like(r), np.zeros_like(r)
    carry = np.zeros_like(lv) if use_gae else lv.copy()
    for t in reversed(range(T)):
        d_next, v_next = (ld, lv) if t == T - 1 else (d[t + 1], v[t + 1])
        nnt = f(1) - d_next
        if use_gae:
            delta = (r[t] + (g * v_next) * nnt) - v[t]
            carry = delta + (gl * nnt) * carry
            adv[t], ret[t] = carry, carry + v[t]
        else:
            carry = r[t] + (g * nnt) * carry
            ret[t], adv[t] = carry, carry - v[t]
    assert adv.dtype == f and ret.dtype == f and carry.dtype == f
    return adv, ret


def gae_torch_loop(rewards, values, dones, next_value, next_done, gamma=0.99, gae_lambda=0.95, use_gae=True):
    """The advantage loop in the reference's form: python-float gamma / lambda times float32 tensors,
    one torch op per operation, on the tensors' device; dones float32."""
    import torch

    num_steps = rewards.shape[0]
    last_value = next_value.reshape(1, -1)
    if use_gae:
        advantages = torch.zeros_like(rewards)
        lastgaelam = 0
        for t in reversed(range(num_steps)):
            if t == num_steps - 1:
                nextnonterminal, nextvalues = 1.0 - next_done, last_value
            else:
                nextnonterminal, nextvalues = 1.0 - dones[t + 1], values[t + 1]
            delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
            advantages[t] = lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
        returns = advantages + values
    else:
        returns = torch.zeros_like(rewards)
        for t in reversed(range(num_steps)):
            if t == num_steps - 1:
                nextnonterminal, next_return = 1.0 - next_done, last_value
            else:
                nextnonterminal, next_return = 1.0 - dones[t + 1], returns[t + 1]
            returns[t] = rewards[t] + gamma * nextnonterminal * next_return
        advantages = returns - values
    return advantages, returns


def gae_inputs(T, N, seed, ends=()):
    """Random float32 rewards / values, dones with about one episode end in eight plus the given
    (t, env) ends (t == T: in last_done), as numpy arrays: rewards, values, dones, last_value, last_done."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, N)).astype(np.float32) * np.float32(3)
    v = rng.standard_normal((T, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.125).astype(np.float32)
    lv = rng.standard_normal(N).astype(np.float32)
    ld = (rng.random(N) < 0.25).astype(np.float32)
    for t, e in ends:
        if t == T:
            ld[e] = 1
        else:
            d[t, e] = 1
    return r, v, d, lv, ld


def discount_bound(raw_rows):
    """Per column of an episode's [L, 7] rows x_t (the six raw rewards and their sum): the bound
    (L + 2) * 2^-23 * sum_t |x_t| between sum_t float32(gamma ** float32(t)) * x_t, as the host
    wrappers compute it, and the contract's float64 product chain.  A float32 power of a float32-
    rounded base carries at most (t + 1) half-ulps of relative error against gamma^t, half an ulp
    more for its own rounding: below (L + 2) * 2^-24 < (L + 2) * 2^-23 relative, per term; the float64
    roundings on either side are 2^-29 times smaller."""
    x = np.abs(np.asarray(raw_rows, np.float64))
    return (x.shape[0] + 2) * 2.0 ** -23 * x.sum(0)
