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

import time

import numpy as np
import torch

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.util.optim import FlatAdamW


class TrainSACAgent(OffPolicyAgent):
    nets = ("network", "critic", "target_critic")
    log_line = "loss actor %8.4f | loss critic %8.4f | reward %8.4f | alpha %8.4f | t %8.4f"
    log_keys = ("loss_actor", "loss_critic", "train_episode_reward", "alpha", "time")

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

    def _explore_action(self):
        """Uniformly random actions (:121-122): the env's own ``action_space.sample()`` where it has one."""
        space = getattr(self.venv, "action_space", None)
        if space is not None:
            return np.asarray(space.sample(), dtype=np.float32).reshape(self.n_envs, self.act_steps, self.action_dim)
        return np.random.uniform(-1.0, 1.0, size=(self.n_envs, self.act_steps, self.action_dim)).astype(np.float32)

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

    def run(self):
        model, dev = self.model, self.device
        E = self.n_envs
        t_start = time.time()
        run_results = []
        cnt_train_step = 0
        done_venv = np.zeros(E, dtype=bool)
        prev_obs = None
        losses = None
        while self.itr < self.n_train_itr:
            eval_mode = self.itr % self.val_freq == 0 and self.itr > self.n_explore_steps and not self.force_train
            n_steps = self.n_steps if not eval_mode else int(1e5)  # an evaluation ends by its episode count
            model.eval() if eval_mode else model.train()
            firsts, rewards = [np.zeros(E)], []
            if self.reset_at_iteration or eval_mode or prev_obs is None:
                prev_obs = self.reset_env_all()
                firsts[0] = np.ones(E)
            else:
                firsts[0] = done_venv.astype(np.float64)
            cnt_episode = 0
            # ---------------- rollout (:117-171)
            for step in range(n_steps):
                state = torch.from_numpy(prev_obs["state"]).float().to(dev)
                if self.itr < self.n_explore_steps:
                    action = self._explore_action()
                else:
                    action = model(cond={"state": state}, deterministic=eval_mode).cpu().numpy()[:, :self.act_steps]
                prev_obs, reward, done_venv = self.env_step(state, action, action, eval_mode)
                rewards.append(np.asarray(reward, dtype=np.float64))
                firsts.append(done_venv.astype(np.float64))
                if not eval_mode:
                    cnt_train_step += E * self.act_steps
                cnt_episode += int(np.sum(done_venv))
                if eval_mode and cnt_episode >= self.n_eval_episode:
                    break
            stats = self._episode_stats(np.stack(firsts), np.stack(rewards))
            # ---------------- update (:209-280)
            if not eval_mode and self.itr > self.n_explore_steps and self.itr % self.critic_update_freq == 0:
                inds = np.random.choice(len(self.replay), self.batch_size, replace=False)
                inds = torch.from_numpy(inds.astype(np.int64)).to(dev)
                losses = self.update_minibatch(inds, update_actor=self.itr % self.actor_update_freq == 0)
            # ---------------- checkpoint, logging (:282-335)
            if self.itr % self.save_model_freq == 0 or self.itr == self.n_train_itr - 1:
                self.save_model()
            rec = {"itr": self.itr, "step": cnt_train_step}
            if self.itr % self.log_freq == 0 and self.itr > self.n_explore_steps:
                fields = {}
                if not eval_mode and losses is not None:  # the only device reads of the loop, on logging iterations
                    fields.update(loss_critic=float(losses[0]), alpha=float(self.log_alpha.detach().exp()))
                    if losses[1] is not None:
                        fields["loss_actor"] = float(losses[1])
                self.log_record(run_results, rec, t_start, eval_mode, stats, fields)
            else:
                run_results.append(rec)
            self.itr += 1
        return run_results
