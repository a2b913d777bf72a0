"""IBRL agent.

Mirrors the reference's ``TrainIBRLAgent`` (agent/finetune/train_ibrl_agent.py:22-354): same cfg keys, same iteration structure.  One
env.  The WHOLE offline dataset is loaded into the replay buffer before the loop, in dataset order and with its rewards unscaled
(:91-105); online transitions follow with ``scale_reward_factor`` applied, and ``buffer_size`` evicts the oldest.  Actions always come
from ``model(cond, deterministic=eval_mode)`` (:149-163): IBRL never acts at random, ``n_explore_steps`` only gates evaluation, update
and log line, all three with ``itr > n_explore_steps`` (:127, :241, :314).  Every ``update_freq`` iterations (:242) the update runs
``critic_num_update`` times [a batch of ``batch_size`` indices drawn with replacement from the one buffer, critic loss and step,
Polyak of the target members], then ONE actor loss and step on the LAST batch and the Polyak of the target actor (:245-297).  Both
cosine schedules are stepped every iteration (:300-301).  Same checkpoint format.

The buffer is the device-resident ring of the other off-policy agents: a batch is an index vector, both losses read their rows
straight off the ring, and every loss, gradient, optimiser step and Polyak average is a library call.  Nothing in
``update_iteration`` reads the device.  The optimiser steps the flat [E][P] image of ``critic_networks`` (the reference steps stacked
copies and leaves ``critic_networks`` at their initial values: model/rl/gaussian_ibrl.py).  State observations only.

Deviation from the reference, documented and not imitated: its log line (:337) and wandb record read ``loss_actor`` / ``loss_critic``
on every logging iteration past ``n_explore_steps``, bound or not -- with ``update_freq`` > 1 the first such iteration can come before
any update and raises an unbound-name error.  Here those fields are left out of the record until an update has run."""
from __future__ import annotations

import numpy as np
import torch

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.cfg.loader import instantiate
from dppo_amd.util.optim import FlatAdamW


class TrainIBRLAgent(OffPolicyAgent):
    nets = ("network", "target_actor", "bc_policy", "_ens", "_tens")  # load() refreshes every kernel image
    strictly_past_exploration = ("eval", "update", "log")
    explores_at_random = False

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "IBRL")
        assert self.n_envs == 1, "IBRL runs one env (every shipped ibrl_mlp*.yaml: env.n_envs = 1)"
        # ---- TrainIBRLAgent (:23-81), in its order
        self.dataset_offline = instantiate(cfg.offline_dataset)
        m = self.model
        self.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, cfg.train.actor_lr_scheduler, cfg.train.actor_lr)
        self.critic_optimizer = FlatAdamW(m.critic_flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        self.critic_lr_scheduler = self._cosine(self.critic_optimizer, cfg.train.critic_lr_scheduler, cfg.train.critic_lr)
        self.target_ema_rate = cfg.train.target_ema_rate
        self.critic_num_update = cfg.train.critic_num_update
        self.update_freq = cfg.train.update_freq
        self.n_eval_episode = cfg.train.n_eval_episode
        self.n_explore_steps = cfg.train.n_explore_steps

    # -------------------------------------------------------------------------------------------------
    def preload_offline(self):
        """The whole offline dataset into the ring, in dataset order, rewards as they are (:91-105)."""
        ds = self.dataset_offline
        b = ds.gather(torch.arange(len(ds), device=self.device))
        n = len(ds)
        self.replay.extend(b.conditions["state"].reshape(n, 1, -1), b.conditions["next_state"].reshape(n, 1, -1),
                           b.actions.reshape(n, 1, -1), b.rewards.reshape(n, 1), b.dones.reshape(n, 1))

    def draw_batch(self):
        """``batch_size`` indices into the one buffer, with replacement, from the global numpy generator (:247)."""
        inds = np.random.choice(len(self.replay), self.batch_size)
        return torch.from_numpy(inds.astype(np.int64)).to(self.device)

    def update_iteration(self, batches=None, pairs=None, critic_draws=None, actor_noise=None, actor_mask=None):
        """One iteration's update in the reference's order (:245-297).  ``critic_num_update`` times: a batch (``batches[i]``, or
        ``draw_batch()``: an index vector into the ring), critic loss and step, Polyak of the target members.  Then ONE actor loss
        and step on the LAST batch, and the Polyak of the target actor.  Nothing here reads the device.  Returns (last critic loss,
        actor loss) as device scalars.  ``pairs[i]`` (the target pair), ``critic_draws[i]`` (a dict of ``loss_critic``'s ``noise_*`` /
        ``mask_*`` / ``next_actions_*``), ``actor_noise`` and ``actor_mask`` replace the draws."""
        m, rp = self.model, self.replay
        pick = lambda x, i: None if x is None else x[i]
        for i in range(self.critic_num_update):
            inds = batches[i] if batches is not None else self.draw_batch()
            loss_c = m.loss_critic(rp, None, None, None, None, self.gamma, inds=inds, pair=pick(pairs, i),
                                   **(pick(critic_draws, i) or {})).detach()
            self.critic_optimizer.step(m.critic_flat_grads())
            m.critics_updated()
            m.update_target_critic(self.target_ema_rate)
        loss_a = m.loss_actor(rp, inds, noise=actor_noise, mask=actor_mask).detach()
        self.actor_optimizer.step(m.last_loss_grad)
        m.network.mark_updated()
        m.update_target_actor(self.target_ema_rate)
        return loss_c, loss_a

    def _update(self):
        """(:239-243) only every ``update_freq`` iterations."""
        if self.itr % self.update_freq:
            return None
        return self.update_iteration()

    def _train_fields(self, losses):
        """No temperature: the two losses of the last update that ran."""
        return dict(loss_critic=float(losses[0]), loss_actor=float(losses[1]))

    def run(self):
        self.preload_offline()
        return self.run_by_episode_count()
