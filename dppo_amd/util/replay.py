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
