"""RLPD agent.

Mirrors the reference's ``TrainRLPDAgent`` (agent/finetune/train_rlpd_agent.py:22-404): same cfg keys, same iteration structure
(``n_steps`` env steps per iteration -- uniformly random actions for the first ``n_explore_steps`` iterations --, FIFO replay,
evaluation by episode count every ``val_freq`` iterations FROM ``n_explore_steps`` on (``>=``, where SAC has ``>``); past the
exploration phase ``critic_num_update`` critic updates per iteration, each on a fresh batch whose first half is drawn from the
offline dataset and whose second half from the replay buffer (``np.random.choice`` with replacement, offline first) and each
followed by the Polyak average, then ONE actor update and one temperature update on the LAST batch, with the temperature's last
snapshot), same checkpoint format.  Both cosine schedules are stepped every iteration.

The offline dataset and the replay buffer are device-resident; a batch is two gathers and one concatenation on the device.  Every
loss, gradient, optimiser step and the Polyak average is a library call; the temperature's snapshot is a device scalar where the
reference reads it back with ``.item()``: nothing in ``update_iteration`` reads the device.  ``log_alpha`` is a device float64 tensor
stepped by ``torch.optim.Adam``.  The optimiser steps the flat [E][P] image of ``critic_networks`` (the reference steps stacked
copies and leaves ``critic_networks`` at their initial values: model/rl/gaussian_rlpd.py).  State observations only.
"""
from __future__ import annotations

import numpy as np
import torch

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.cfg.loader import instantiate
from dppo_amd.util.optim import FlatAdamW


class TrainRLPDAgent(OffPolicyAgent):
    nets = ("network", "_ens", "_tens")  # the actor and both ensembles: load() refreshes every kernel image
    log_line = "loss actor %8.4f | loss critic %8.4f | reward %8.4f | alpha %8.4f | t %8.4f"
    log_keys = ("loss_actor", "loss_critic", "train_episode_reward", "alpha", "time")

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "RLPD")
        # ---- TrainRLPDAgent (:23-88), in its order
        self.dataset_offline = instantiate(cfg.offline_dataset)
        m = self.model
        self.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, cfg.train.actor_lr_scheduler, cfg.train.actor_lr)
        self.critic_optimizer = FlatAdamW(m.critic_flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        self.critic_lr_scheduler = self._cosine(self.critic_optimizer, cfg.train.critic_lr_scheduler, cfg.train.critic_lr)
        self.target_ema_rate = cfg.train.target_ema_rate
        self.critic_num_update = cfg.train.critic_num_update
        self.n_eval_episode = cfg.train.n_eval_episode
        self.n_explore_steps = cfg.train.n_explore_steps
        self.log_alpha = torch.tensor(np.log(cfg.train.init_temperature), dtype=torch.float64, device=self.device,
                                      requires_grad=True)
        self.target_entropy = cfg.train.target_entropy
        self.log_alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=cfg.train.critic_lr)

    # -------------------------------------------------------------------------------------------------
    def draw_batch(self):
        """One batch (:251-310): ``batch_size // 2`` offline transitions, then as many from the replay buffer, both drawn with
        replacement from the global numpy generator in that order, gathered and concatenated on the device."""
        half, dev = self.batch_size // 2, self.device
        off_i = np.random.choice(len(self.dataset_offline), half)
        on_i = np.random.choice(len(self.replay), half)
        off = self.dataset_offline.gather(torch.from_numpy(off_i.astype(np.int64)).to(dev))
        on = self.replay.gather(torch.from_numpy(on_i.astype(np.int64)).to(dev))
        flat = lambda x: x.reshape(half, -1).float()
        cat = lambda a, b: torch.cat([a, b], dim=0)
        return dict(obs=cat(flat(off.conditions["state"]), flat(on[0])), next_obs=cat(flat(off.conditions["next_state"]), flat(on[1])),
                    actions=cat(flat(off.actions), flat(on[2])), reward=cat(off.rewards.reshape(half).float(), on[3].reshape(half)),
                    terminated=cat(off.dones.reshape(half).float(), on[4].reshape(half)))

    def update_iteration(self, batches=None, pairs=None, next_actions=None, next_logp=None, sample_noise=None, actor_noise=None,
                         temp_noise=None):
        """One iteration's update in the reference's order (:246-347).  ``critic_num_update`` times: a batch (``batches[i]``, or
        ``draw_batch()``), the temperature's snapshot, critic loss and step, Polyak.  Then ONE actor loss and step on the LAST
        batch with the last snapshot, the temperature loss on a fresh sample at that batch and its step.  Nothing here reads the
        device.  Returns (last critic loss, actor loss, temperature loss) as device scalars.  ``pairs[i]`` (the target pair),
        ``next_actions[i]`` + ``next_logp[i]`` or ``sample_noise[i]`` (the critic loss's sample / its draws), ``actor_noise`` and
        ``temp_noise`` replace the draws."""
        m = self.model
        pick = lambda x, i: None if x is None else x[i]
        for i in range(self.critic_num_update):
            b = batches[i] if batches is not None else self.draw_batch()
            alpha = self.log_alpha.detach().exp()
            loss_c = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], self.gamma,
                                   alpha, next_actions=pick(next_actions, i), next_logp=pick(next_logp, i),
                                   noise=pick(sample_noise, i), pair=pick(pairs, i)).detach()
            self.critic_optimizer.step(m.critic_flat_grads())
            m.critics_updated()
            m.update_target_critic(self.target_ema_rate)
        loss_a = m.loss_actor({"state": b["obs"]}, alpha, noise=actor_noise).detach()
        self.actor_optimizer.step(m.last_loss_grad)
        m.network.mark_updated()
        self.log_alpha_optimizer.zero_grad()
        lt = m.loss_temperature({"state": b["obs"]}, self.log_alpha, self.target_entropy, noise=temp_noise)
        lt.backward()
        self.log_alpha_optimizer.step()
        return loss_c, loss_a, lt.detach()

    run = OffPolicyAgent.run_by_episode_count  # (:154-404) with its defaults
