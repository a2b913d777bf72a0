"""Device-resident FIFO replay buffer of the off-policy agents (reference agent/finetune/train_idql_diffusion_agent.py:101-105,
178-182, 233-253: five ``deque(maxlen=buffer_size)`` of per-step arrays, copied to numpy and flattened ``"s e ... -> (s e) ..."``
before every update).  Here the five arrays are rings of ``buffer_size`` steps that never leave the device; the library's row
builder (csrc/idql.hip) gathers a minibatch straight out of them from an index vector over the same logical order."""
from __future__ import annotations

import numpy as np
import torch

from dppo_amd import hip


class DeviceReplay:
    """Ring of ``buffer_size`` steps of ``n_envs`` transitions.  Logical index ``i = s * n_envs + e`` counts the stored steps
    oldest first (what the reference's flattened deque holds at position ``i``); step ``s`` lives in slot
    ``(head + s) % buffer_size``."""

    def __init__(self, buffer_size: int, n_envs: int, obs_dim: int, act_dim: int, device="cuda:0"):
        self.cap, self.n_envs, self.obs_dim, self.act_dim = int(buffer_size), int(n_envs), int(obs_dim), int(act_dim)
        kw = dict(dtype=torch.float32, device=device)
        self.obs = torch.zeros(self.cap, self.n_envs, self.obs_dim, **kw)
        self.next_obs = torch.zeros(self.cap, self.n_envs, self.obs_dim, **kw)
        self.actions = torch.zeros(self.cap, self.n_envs, self.act_dim, **kw)
        self.reward = torch.zeros(self.cap, self.n_envs, **kw)
        self.terminated = torch.zeros(self.cap, self.n_envs, **kw)
        self.head, self.steps = 0, 0

    def __len__(self) -> int:
        return self.steps * self.n_envs

    def append(self, prev_obs, next_obs, action, reward, terminated) -> None:
        """One env step of all envs; the oldest step is evicted when the ring is full (``deque(maxlen)``)."""
        if self.steps < self.cap:
            slot = (self.head + self.steps) % self.cap
            self.steps += 1
        else:
            slot = self.head
            self.head = (self.head + 1) % self.cap
        for dst, src in ((self.obs, prev_obs), (self.next_obs, next_obs), (self.actions, action), (self.reward, reward),
                         (self.terminated, terminated)):
            dst[slot].copy_(torch.as_tensor(np.asarray(src) if not torch.is_tensor(src) else src).reshape(dst[slot].shape),
                            non_blocking=True)

    def extend(self, prev_obs, next_obs, action, reward, terminated) -> None:
        """T env steps at once, each argument with a leading dimension T: what T calls of ``append`` in that order leave behind,
        wrap-around and eviction included (``deque.extend``), in one indexed copy per array.  A subclass with an ``append`` of its
        own is fed step by step."""
        srcs = [torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x) for x in (prev_obs, next_obs, action, reward, terminated)]
        T = int(srcs[0].shape[0])
        if type(self).append is not DeviceReplay.append:
            for t in range(T):
                self.append(*[x[t] for x in srcs])
            return
        if T == 0:
            return
        first = (self.head + self.steps) % self.cap  # where the first new step goes, full or not
        live = min(T, self.cap)                      # only the last ``cap`` new steps survive
        slots = ((first + torch.arange(T - live, T)) % self.cap).to(self.obs.device)
        for dst, src in zip((self.obs, self.next_obs, self.actions, self.reward, self.terminated), srcs):
            rows = src[T - live:].reshape(live, *dst.shape[1:]).to(device=dst.device, dtype=dst.dtype, non_blocking=True)
            dst.index_copy_(0, slots, rows)
        total = self.steps + T
        if total > self.cap:
            self.head = (self.head + total - self.cap) % self.cap
        self.steps = min(total, self.cap)

    def slot_of(self, inds: torch.Tensor) -> torch.Tensor:
        """Storage row (slot * n_envs + e) of each logical index: the mapping the row builder applies on the device."""
        s, e = torch.div(inds, self.n_envs, rounding_mode="floor"), inds % self.n_envs
        return ((self.head + s) % self.cap) * self.n_envs + e

    def gather(self, inds: torch.Tensor):
        """(obs, next_obs, actions, reward, terminated) rows of the logical indices ``inds`` as tensors (tests, logging)."""
        rows = self.slot_of(inds.to(self.obs.device))
        return tuple(t.reshape(self.cap * self.n_envs, *t.shape[2:])[rows]
                     for t in (self.obs, self.next_obs, self.actions, self.reward, self.terminated))

    def draw(self, num_batch: int, batch_size: int) -> torch.Tensor:
        """The indices of ``num_batch`` minibatches, drawn on the host like the reference (``np.random.choice(len, batch_size)``
        per minibatch: the same stream of the global numpy generator) and uploaded once."""
        inds = np.random.choice(len(self), (num_batch, batch_size))
        return torch.from_numpy(inds.astype(np.int64)).to(self.obs.device)

    def batch(self, inds=None) -> "hip.IdqlBatch":
        """The ``dppo_idql_batch`` of this ring for one library call; ``inds``: (N,) int64 device tensor (kept alive by the
        caller until the call is queued) or None for the identity."""
        return hip.IdqlBatch(self.obs.data_ptr(), self.next_obs.data_ptr(), self.actions.data_ptr(), self.reward.data_ptr(),
                             self.terminated.data_ptr(), None if inds is None else inds.data_ptr(), self.cap, self.n_envs,
                             self.head, self.steps)


class ReturnsReplay(DeviceReplay):
    """``DeviceReplay`` with a sixth column: the Monte-Carlo reward-to-go of every stored transition (Cal-QL's online half; reference
    agent/finetune/train_calql_agent.py:109, 258-276).  A return is known only when its episode ends, so ``append`` remembers the
    slots of every env's OPEN episode and ``close_episode`` writes that episode's discounted returns into exactly those slots: a
    return lives in its transition's slot, so wrap-around and eviction cannot separate the two.  Only transitions of closed episodes
    are drawn (``closed_indices`` / ``draw``); the bookkeeping is host-side numpy, nothing here reads the device.  An episode longer
    than the ring would evict its own head before its return is known: that is an error."""

    def __init__(self, buffer_size: int, n_envs: int, obs_dim: int, act_dim: int, device="cuda:0"):
        super().__init__(buffer_size, n_envs, obs_dim, act_dim, device)
        self.reward_to_go = torch.zeros(self.cap, self.n_envs, dtype=torch.float32, device=device)
        self.closed = np.zeros((self.cap, self.n_envs), dtype=bool)  # slot holds a transition whose return is written
        self.open_slots = [[] for _ in range(self.n_envs)]           # per env: the open episode's slots, oldest first

    def append(self, prev_obs, next_obs, action, reward, terminated) -> None:
        slot = (self.head + self.steps) % self.cap if self.steps < self.cap else self.head
        for e, op in enumerate(self.open_slots):
            if op and op[0] == slot:
                raise ValueError(f"an episode of env {e} is longer than the replay ring ({self.cap} steps): its first transition "
                                 "would be evicted before its return is known")
        super().append(prev_obs, next_obs, action, reward, terminated)
        self.closed[slot] = False
        for op in self.open_slots:
            op.append(slot)

    def close_episode(self, returns, env: int = 0) -> None:
        """The episode of ``env`` that is open ends: ``returns`` (its length,) are the discounted rewards-to-go of its transitions,
        oldest first, computed on the host from the rollout's rewards."""
        slots = self.open_slots[env]
        returns = np.asarray(returns, dtype=np.float32).reshape(-1)
        if len(returns) != len(slots):
            raise ValueError(f"close_episode: {len(returns)} returns for the {len(slots)} transitions of env {env}'s open episode")
        if len(slots):
            rows = torch.as_tensor(np.asarray(slots, dtype=np.int64))
            self.reward_to_go[rows.to(self.reward_to_go.device), env] = torch.from_numpy(returns).to(self.reward_to_go.device)
            self.closed[slots, env] = True
        self.open_slots[env] = []

    def closed_indices(self) -> np.ndarray:
        """The logical indices (oldest first) of the stored transitions whose episode is closed."""
        order = (self.head + np.arange(self.steps)) % self.cap
        return np.flatnonzero(self.closed[order].reshape(-1))

    def n_closed(self) -> int:
        return int(self.closed.sum())

    def gather(self, inds: torch.Tensor):
        """(obs, next_obs, actions, reward, terminated, reward_to_go) rows of the logical indices ``inds``."""
        rows = self.slot_of(inds.to(self.obs.device))
        return super().gather(inds) + (self.reward_to_go.reshape(self.cap * self.n_envs)[rows],)

    def draw(self, num_batch: int, batch_size: int) -> torch.Tensor:
        """As ``DeviceReplay.draw`` over the transitions of closed episodes only."""
        ok = self.closed_indices()
        inds = ok[np.random.choice(len(ok), (num_batch, batch_size))]
        return torch.from_numpy(inds.astype(np.int64)).to(self.obs.device)
