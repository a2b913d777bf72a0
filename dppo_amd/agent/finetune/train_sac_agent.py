"""SAC agent.

Mirrors the reference's ``TrainSACAgent`` (agent/finetune/train_sac_agent.py:20-335): same cfg keys, same iteration structure
(``n_steps`` env steps per iteration -- uniformly random actions for the first ``n_explore_steps`` iterations --, FIFO replay,
evaluation by episode count every ``val_freq`` iterations; past the exploration phase one critic update every
``batch_size / critic_replay_ratio`` iterations, the Polyak average behind it, and every ``batch_size / actor_replay_ratio``
iterations two actor + temperature updates on the same minibatch, with the temperature read ONCE before the critic update and
reused for both), same checkpoint format.  As in the other off-policy agents the replay buffer is a device-resident ring and every
loss, gradient, optimiser step and the Polyak average is a library call.  Where the reference reads alpha back with ``.item()``
once per update, the snapshot here is a device scalar: nothing in ``update_minibatch`` reads the device.  ``log_alpha`` is a
device float64 tensor stepped by ``torch.optim.Adam``.  State observations only, like the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.util.optim import FlatAdamW


class TrainSACAgent(OffPolicyAgent):
    nets = ("network", "critic", "target_critic")
    log_line = "loss actor %8.4f | loss critic %8.4f | reward %8.4f | alpha %8.4f | t %8.4f"
    log_keys = ("loss_actor", "loss_critic", "train_episode_reward", "alpha", "time")
    lr_schedulers = ()  # (:21-68 builds none)
    strictly_past_exploration = ("eval", "update", "log")

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "SAC")
        # ---- TrainSACAgent (:21-68); torch.optim.Adam there is AdamW without decay here
        m = self.model
        self.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=cfg.train.actor_lr, weight_decay=0)
        self.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=cfg.train.critic_lr, weight_decay=0)
        self.target_ema_rate = cfg.train.target_ema_rate
        self.critic_update_freq = int(cfg.train.batch_size / cfg.train.critic_replay_ratio)
        self.actor_update_freq = int(cfg.train.batch_size / cfg.train.actor_replay_ratio)
        self.n_eval_episode = cfg.train.n_eval_episode
        self.n_explore_steps = cfg.train.n_explore_steps
        self.log_alpha = torch.tensor(np.log(cfg.train.init_temperature), dtype=torch.float64, device=self.device,
                                      requires_grad=True)
        self.target_entropy = cfg.train.target_entropy
        self.log_alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=cfg.train.critic_lr)

    # -------------------------------------------------------------------------------------------------
    def update_minibatch(self, inds, update_actor=True, next_actions=None, next_logp=None, sample_noise=None, actor_noise=None,
                         temp_noise=None):
        """One update in the reference's order (:242-280): the temperature's snapshot; critic loss and step; Polyak; then, when
        ``update_actor``, twice: actor loss with the snapshot and the UPDATED critic, actor step, temperature loss and step.
        Nothing here reads the device.  Returns (critic loss, last actor loss or None, last temperature loss or None) as device
        scalars.  ``next_actions`` + ``next_logp`` / ``sample_noise`` (the critic loss's sample / its draws) and ``actor_noise``,
        ``temp_noise`` (one tensor per actor / temperature update) replace the draws."""
        m, rp = self.model, self.replay
        alpha = self.log_alpha.detach().exp()
        loss_c = m.loss_critic(rp, None, None, None, None, self.gamma, alpha, inds=inds, next_actions=next_actions,
                               next_logp=next_logp, noise=sample_noise).detach()
        self.critic_optimizer.step(m.critic.flat_grads())
        m.critic.mark_updated()
        m.update_target_critic(self.target_ema_rate)
        loss_a = loss_t = None
        if update_actor:
            for i in range(2):
                loss_a = m.loss_actor(rp, alpha, inds=inds, noise=None if actor_noise is None else actor_noise[i]).detach()
                self.actor_optimizer.step(m.last_loss_grad)
                m.network.mark_updated()
                self.log_alpha_optimizer.zero_grad()
                lt = m.loss_temperature(rp, self.log_alpha, self.target_entropy, inds=inds,
                                        noise=None if temp_noise is None else temp_noise[i])
                lt.backward()
                self.log_alpha_optimizer.step()
                loss_t = lt.detach()
        return loss_c, loss_a, loss_t

    def _update(self):
        """(:209-280) one critic update every ``critic_update_freq`` iterations, the actor's with it every ``actor_update_freq``."""
        if self.itr % self.critic_update_freq:
            return None
        inds = np.random.choice(len(self.replay), self.batch_size, replace=False)
        inds = torch.from_numpy(inds.astype(np.int64)).to(self.device)
        return self.update_minibatch(inds, update_actor=self.itr % self.actor_update_freq == 0)

    run = OffPolicyAgent.run_by_episode_count
