"""A plain-Python restatement of the episode monitor (include/miniworld_batch.h at mwb_monitor_enable), independent of the kernels:
the trainer's loop over the envs after every step

    for idx, eps_done in enumerate(done):
        if eps_done: episode_rewards.append(...)                 (pytorch-a2c-ppo-acktr/main.py:167-169, deque(maxlen=100) :141)

with the return summed per episode (Python floats, added in step order: comparisons with the device are bit equality), a
collections.deque(maxlen=capacity) of (return, len, calls, env), the partial / skip / quota rules and the evaluation table."""
import math
from collections import deque


class MonitorRef:
    def __init__(self, num_envs, capacity, quota_max=0):
        n = self.n = int(num_envs)
        self.capacity, self.quota_max = int(capacity), int(quota_max)
        self.run_return, self.run_len, self.run_calls = [0.0] * n, [0] * n, [0] * n
        self.partial, self.finished, self.retired, self.logged = [False] * n, [0] * n, [False] * n, [False] * n
        self.last_return, self.last_len, self.last_calls = [0.0] * n, [0] * n, [0] * n
        self.log = deque(maxlen=self.capacity)
        self.total = self.dropped = 0
        self.quota, self.remaining = 0, n
        self._fill_table()

    def _fill_table(self):
        self.tab_return = [[math.nan] * self.n for _ in range(self.quota_max)]
        self.tab_len = [[-1] * self.n for _ in range(self.quota_max)]

    def update(self, reward, done, taken=None, skip=None):
        """one pass; returns how many episodes it logged"""
        logged = 0
        self.logged = [False] * self.n
        for e in range(self.n):
            if skip is not None and skip[e]:
                continue   # untouched: its reward of -99 enters no return
            self.run_return[e] = self.run_return[e] + float(reward[e])
            self.run_len[e] += 1 if taken is None else int(taken[e])
            self.run_calls[e] += 1
            if done[e]:
                if self.partial[e]:
                    self.dropped += 1
                else:
                    rec = (self.run_return[e], self.run_len[e], self.run_calls[e], e)
                    self.last_return[e], self.last_len[e], self.last_calls[e] = rec[:3]
                    self.log.append(rec)
                    self.total += 1
                    logged += 1
                    self.logged[e] = True
                    if self.finished[e] < self.quota_max:
                        self.tab_return[self.finished[e]][e] = rec[0]
                        self.tab_len[self.finished[e]][e] = rec[1]
                    self.finished[e] += 1
                self.run_return[e], self.run_len[e], self.run_calls[e] = 0.0, 0, 0
                self.partial[e] = False
        self.retired = [self.quota > 0 and f >= self.quota for f in self.finished]
        self.remaining = self.retired.count(False)
        return logged

    def clear(self, mask=None, partial=False):
        for e in range(self.n):
            if mask is None or mask[e]:
                self.run_return[e], self.run_len[e], self.run_calls[e] = 0.0, 0, 0
                self.partial[e] = bool(partial)

    def set_quota(self, q):
        assert 0 <= q <= self.quota_max
        self.quota = int(q)
        self.finished, self.retired, self.remaining = [0] * self.n, [False] * self.n, self.n
        self._fill_table()


def assert_equal(mon, ref, what=""):
    """every per-env array, the log read oldest first, the counters and the table of a gym_miniworld_amd Monitor equal the
    reference's exactly (returns as float64 bit patterns, NaN cells included)"""
    import numpy as np
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.int64)   # noqa: E731
    host = lambda t: t.cpu().numpy()   # noqa: E731
    assert mon.read() == (ref.total, ref.dropped, ref.remaining), (what, mon.read(), (ref.total, ref.dropped, ref.remaining))
    for name in ("run_return", "last_return"):
        assert np.array_equal(bits(host(getattr(mon, name))), bits(getattr(ref, name))), (what, name)
    for name in ("run_len", "run_calls", "last_len", "last_calls", "finished"):
        assert np.array_equal(host(getattr(mon, name)), np.asarray(getattr(ref, name), np.int32)), (what, name)
    for name in ("partial", "retired", "logged"):
        assert np.array_equal(host(getattr(mon, name)) != 0, np.asarray(getattr(ref, name), bool)), (what, name)
    r, ln, calls, envs = (host(t) for t in mon.log())
    want = list(ref.log)
    assert len(r) == len(want), (what, len(r), len(want))
    assert np.array_equal(bits(r), bits([w[0] for w in want])), (what, "log returns")
    assert ln.tolist() == [w[1] for w in want] and calls.tolist() == [w[2] for w in want] and envs.tolist() == [w[3] for w in want], (what, "log")
    if ref.quota_max:
        assert np.array_equal(bits(host(mon.tab_return)), bits(ref.tab_return)), (what, "tab_return")
        assert np.array_equal(host(mon.tab_len), np.asarray(ref.tab_len, np.int32)), (what, "tab_len")
