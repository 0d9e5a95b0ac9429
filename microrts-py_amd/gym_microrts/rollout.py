"""The bookkeeping around step() on the tensor contract, on the device (csrc/mrts_rollout.hip).

`EpisodeStats` is the reference's VecMonitor + MicroRTSStatsRecorder pair (ppo_gridnet.py:126-160,
384-385) for `return_tensors=True`: fed the tensors step() returns, it keeps every env's running
episode return, length and per-reward-function sums in HBM and appends one record per finished
episode to a device ring, in the order the reference's `for info in infos` scan meets them.
Nothing is read on the host until `drain()`.

    stats = rollout.EpisodeStats.for_env(envs, gamma=0.99)
    obs, reward, done, infos = envs.step(actions)
    stats.update(reward, done, infos)             # one launch, no sync
    for rec in stats.drain():                     # once per update: one sync
        rec["episode"]["r"], rec["episode"]["l"], rec["microrts_stats"]["WinLossRewardFunction"]

`gae` is the advantage loop (ppo_gridnet.py:496-519, both branches) as one launch over the [T, N]
buffers.  The arithmetic of both is stated in include/microrts_amd.h.  There is no CPU path: a CPU
tensor is an error.
"""
import numpy as np
import torch

from . import _native

ROW = _native.MRTS_EPISODE_RECORD_DOUBLES   # float64 per record: env, step, r, l, 6 sums, 7 discounted sums, 0
RAW = 6                                     # reward functions
HEADER_BYTES = 32


def layout(num_envs, capacity):
    """Byte offsets of the state buffer's arrays (include/microrts_amd.h): cnt, ret, len, factor,
    rawsum, disc, ring, and the whole size `bytes`."""
    n = int(num_envs)
    ret = HEADER_BYTES
    length = ret + 4 * n
    factor = length + 4 * n
    rawsum = factor + 8 * n
    disc = rawsum + 48 * n
    ring = (disc + 56 * n + 15) & ~15
    return {"cnt": 0, "ret": ret, "len": length, "factor": factor, "rawsum": rawsum, "disc": disc, "ring": ring,
            "bytes": ring + int(capacity) * ROW * 8}


def ring_span(drained, count, capacity):
    """Which records a drain returns: `drained` records were returned before, `count` were written
    since creation into a ring of `capacity` rows (record k in row k % capacity).  Returns
    (first, dropped, slices): the survivors are records first .. count - 1, `dropped` older ones
    were overwritten, and `slices` lists the (begin, end) row ranges that hold the survivors in order."""
    new = count - drained
    if new < 0 or capacity < 1:
        raise ValueError(f"ring_span: count {count} behind drained {drained}, or capacity {capacity} < 1")
    dropped = max(0, new - capacity)
    first = drained + dropped
    a, b = first % capacity, first % capacity + (count - first)
    if count == first:
        slices = []
    elif b <= capacity:
        slices = [(a, b)]
    else:
        slices = [(a, capacity), (0, b - capacity)]
    return first, dropped, slices


def records_of(rows, names):
    """Ring rows (float64 [k, ROW]) -> the reference's info entries, one dict per row:
    {"env", "step", "episode": {"r", "l"}, "microrts_stats": {name: sum, ..., "discounted_<name>": ..., "discounted": ...}}."""
    names = list(names)
    dnames = ["discounted_" + k for k in names] + ["discounted"]
    out = []
    for row in np.asarray(rows, dtype=np.float64).reshape(-1, ROW):
        stats = dict(zip(names, row[4:4 + RAW]))
        stats.update(zip(dnames, row[4 + RAW:4 + RAW + RAW + 1]))
        out.append({"env": int(row[0]), "step": int(row[1]), "episode": {"r": float(row[2]), "l": int(row[3])},
                    "microrts_stats": stats})
    return out


def _check(t, name, dtypes, shape):
    """Type, dtype, shape and layout; the device is checked once all of a call's tensors passed
    these (_on_gpu), so a shape error names the shape wherever the tensor lives."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, not {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _on_gpu(named, dev=None):
    """Every (name, tensor) on one GPU (`dev`, or the first tensor's)."""
    for name, t in named:
        if t.device.type != "cuda":
            raise ValueError(f"{name} is on {t.device}: the rollout bookkeeping runs on the GPU only (no CPU fallback)")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, not on {dev}")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


BYTES = (torch.bool, torch.uint8)


def check_update(num_envs, reward, done, infos_or_raw, dev=None):
    """EpisodeStats.update's input check; returns the raw-reward tensor (a LazyInfos gives its own
    without materialising anything)."""
    raw = getattr(infos_or_raw, "_raw", infos_or_raw)
    _check(reward, "reward", (torch.float64,), (num_envs,))
    _check(done, "done", BYTES, (num_envs,))
    _check(raw, "raw", (torch.float64,), (num_envs, RAW))
    _on_gpu((("reward", reward), ("done", done), ("raw", raw)), dev)
    return raw


class EpisodeStats:
    """Per-env episode return / length / per-reward-function sums and the ring of finished episodes,
    all in one device buffer.  `names`: the six reward functions' names, `[str(rf) for rf in envs.rfs]`.
    `capacity`: ring rows, default max(4 * num_envs, 1024); when more episodes than that finish between
    two drains the oldest are lost and counted in `.dropped`."""

    def __init__(self, num_envs, names, gamma=0.99, capacity=None, device="cuda"):
        names = [str(k) for k in names]
        if int(num_envs) < 1:
            raise ValueError(f"num_envs must be >= 1, not {num_envs}")
        if len(names) != RAW:
            raise ValueError(f"names must hold the {RAW} reward functions' names, not {len(names)}")
        capacity = max(4 * int(num_envs), 1024) if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity must be >= 1, not {capacity}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device is {self.device}: the rollout bookkeeping runs on the GPU only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs, self.names, self.gamma, self.capacity = int(num_envs), names, float(gamma), capacity
        self.layout = layout(self.num_envs, capacity)
        nbytes = _native.lib().mrts_episode_stats_bytes(self.num_envs, capacity)
        if nbytes != self.layout["bytes"]:
            raise _native.MicroRTSError(f"episode-stats layout: the library says {nbytes} bytes, this module {self.layout['bytes']}")
        self._buf = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        self._ring = self._buf[self.layout["ring"] // 8:].view(torch.float64).view(capacity, ROW)
        self.reset()

    @classmethod
    def for_env(cls, envs, gamma=0.99, capacity=None):
        return cls(envs.num_envs, [str(rf) for rf in envs.rfs], gamma=gamma, capacity=capacity, device=envs.device)

    def reset(self):
        """Every running sum and the ring start afresh; the serial number returns to 0."""
        with torch.cuda.device(self.device):
            rc = _native.lib().mrts_episode_stats_init(_stream(self.device), self._buf.data_ptr(), self.num_envs, self.capacity)
        _native.check(rc, None, "episode_stats_init")
        self.steps = 0      # update() calls so far: the next call's serial number
        self.dropped = 0    # records lost to the ring's wrap-around, over all drains
        self._drained = 0   # records returned or dropped so far

    def update(self, reward, done, infos_or_raw):
        """One env-step's outputs: reward [N] float64, done [N] bool (or uint8), and the infos step()
        returned (its raw rewards are read in place) or the raw rewards [N, 6] float64 themselves.
        One launch on the current stream; nothing is synchronised."""
        n = self.num_envs
        raw = check_update(n, reward, done, infos_or_raw, self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().mrts_episode_stats_update(_stream(self.device), self._buf.data_ptr(), n, self.capacity, self.gamma,
                                                         self.steps, reward.data_ptr(), done.data_ptr(), raw.data_ptr())
        _native.check(rc, None, "episode_stats_update")
        self.steps += 1

    def state(self):
        """The running state as views of the buffer (no copy): ret [N] float32, len [N] int32,
        factor [N], rawsum [6, N], disc [7, N] float64."""
        L, n, b = self.layout, self.num_envs, self._buf
        f64 = b.view(torch.float64)
        return {"ret": b.view(torch.float32)[L["ret"] // 4:L["ret"] // 4 + n], "len": b.view(torch.int32)[L["len"] // 4:L["len"] // 4 + n],
                "factor": f64[L["factor"] // 8:L["factor"] // 8 + n], "rawsum": f64[L["rawsum"] // 8:L["rawsum"] // 8 + 6 * n].view(6, n),
                "disc": f64[L["disc"] // 8:L["disc"] // 8 + 7 * n].view(7, n)}

    def drain_rows(self):
        """The records finished since the last drain as float64 rows [k, ROW] on the host, in record
        order: the counter's copy (the one sync), then the new rows'."""
        count = int(self._buf[self.steps & 1].item())
        _, dropped, slices = ring_span(self._drained, count, self.capacity)
        self.dropped += dropped
        self._drained = count
        if not slices:
            return np.zeros((0, ROW), np.float64)
        parts = [self._ring[a:b] for a, b in slices]
        return (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy()

    def drain(self):
        """The episodes finished since the last drain, as the reference's info entries in its scan
        order (ascending env within a step, step order across): a list of
        {"env", "step", "episode": {"r", "l"}, "microrts_stats": {...}}."""
        return records_of(self.drain_rows(), self.names)


def gae(rewards, values, dones, last_value, last_done, gamma=0.99, gae_lambda=0.95, use_gae=True, out=None):
    """rewards, values [T, N] float32; dones [T, N] and last_done [N], both float32 (what the
    reference stores) or both bool / uint8; last_value [N] float32 -> (advantages, returns),
    [T, N] float32.  use_gae=False: the reference's `--gae False` branch (discounted returns,
    advantages = returns - values).  `out`: a pair of contiguous float32 [T, N] tensors to write into."""
    if not isinstance(rewards, torch.Tensor):
        raise ValueError(f"rewards must be a torch.Tensor, not {type(rewards).__name__}")
    if rewards.dim() != 2 or rewards.shape[0] < 1 or rewards.shape[1] < 1:
        raise ValueError(f"rewards must be [T, N] with T, N >= 1, not {list(rewards.shape)}")
    T, n = rewards.shape
    f32 = (torch.float32,)
    _check(rewards, "rewards", f32, (T, n))
    _check(values, "values", f32, (T, n))
    _check(dones, "dones", f32 + BYTES, (T, n))
    _check(last_value, "last_value", f32, (n,))
    _check(last_done, "last_done", f32 if dones.dtype == torch.float32 else BYTES, (n,))
    named = [("rewards", rewards), ("values", values), ("dones", dones), ("last_value", last_value), ("last_done", last_done)]
    if out is not None:
        adv, ret = out
        _check(adv, "out[0]", f32, (T, n))
        _check(ret, "out[1]", f32, (T, n))
        named += [("out[0]", adv), ("out[1]", ret)]
    dev = _on_gpu(named)
    if out is None:
        adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    elem = _native.MRTS_DONE_FLOAT32 if dones.dtype == torch.float32 else _native.MRTS_DONE_UINT8
    mode = _native.MRTS_GAE_ADVANTAGES if use_gae else _native.MRTS_GAE_RETURNS
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_gae(_stream(dev), T, n, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), elem,
                                    last_value.data_ptr(), last_done.data_ptr(), float(gamma), float(gae_lambda), mode,
                                    adv.data_ptr(), ret.data_ptr())
    _native.check(rc, None, "gae")
    return adv, ret
