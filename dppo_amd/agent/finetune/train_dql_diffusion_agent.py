"""DQL fine-tuning agent.

Mirrors the reference's ``TrainDQLDiffusionAgent`` (agent/finetune/train_dql_diffusion_agent.py:27-300): same cfg keys, same
iteration structure (rollout with the plain sampler -> FIFO replay -> ``n_steps * n_envs / batch_size * replay_ratio``
minibatch updates: critic loss and step, actor loss WITH THE UPDATED critic -- differentiated through the sampling chain --,
actor step after the critic warm-up, Polyak -> LR schedules -> checkpoint), same checkpoint format.  As in the IDQL and QSM agents
the replay buffer is a device-resident ring, the minibatch indices of a whole iteration are drawn on the host once, every loss,
gradient, optimiser step and the Polyak average is a library call, and nothing in the minibatch loop reads the device (the coin of
``loss_actor`` is drawn on the host, like the reference's).  State observations only, like the reference.
"""
from __future__ import annotations

import logging
import os
import pickle
import time

import numpy as np
import torch

from dppo_amd.agent.finetune.train_idql_diffusion_agent import OffPolicyDiffusionAgent
from dppo_amd.util.optim import FlatAdamW
from dppo_amd.util.replay import DeviceReplay
from dppo_amd.util.scheduler import CosineAnnealingWarmupRestarts

log = logging.getLogger(__name__)


class TrainDQLDiffusionAgent(OffPolicyDiffusionAgent):
    def __init__(self, cfg, venv=None):
        self._init_train_agent(cfg, venv, "DQL")
        # ---- TrainDQLDiffusionAgent (:29-81)
        self.gamma = cfg.train.gamma  # applied to the reward of every act_steps env steps
        self.n_critic_warmup_itr = cfg.train.n_critic_warmup_itr
        m = self.model
        self.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        sa, sc = cfg.train.actor_lr_scheduler, cfg.train.critic_lr_scheduler
        mk = lambda opt, s, lr: CosineAnnealingWarmupRestarts(opt, first_cycle_steps=s.first_cycle_steps, cycle_mult=1.0, max_lr=lr,
                                                              min_lr=s.min_lr, warmup_steps=s.warmup_steps, gamma=1.0)
        self.actor_lr_scheduler = mk(self.actor_optimizer, sa, cfg.train.actor_lr)
        self.critic_lr_scheduler = mk(self.critic_optimizer, sc, cfg.train.critic_lr)
        self.buffer_size = cfg.train.buffer_size
        self.scale_reward_factor = cfg.train.scale_reward_factor
        self.replay_ratio = cfg.train.replay_ratio
        self.target_ema_rate = cfg.train.target_ema_rate
        self.eta = cfg.train.eta
        self.replay = DeviceReplay(self.buffer_size, self.n_envs, self.n_cond_step * self.obs_dim,
                                   self.act_steps * self.action_dim, self.device)

    def load(self, itr):
        data = torch.load(os.path.join(self.checkpoint_dir, f"state_{itr}.pt"), weights_only=True)
        self.itr = data["itr"]
        self.model.load_state_dict(data["model"])
        for net in (self.model.actor, self.model.critic, self.model.critic_target):
            net.mark_updated()  # kernel images are rebuilt from the loaded weights on next use

    # -------------------------------------------------------------------------------------------------
    def update_minibatch(self, inds, next_actions=None, sample_noise=None, **actor_draws):
        """One minibatch in the reference's order (:222-260): critic loss and step; actor loss with the UPDATED critic; the
        actor's step (clipped at ``max_grad_norm``) only after the critic warm-up, its loss and gradient either way; Polyak.
        Nothing here reads the device.  Returns the two losses as device scalars.  ``next_actions`` / ``sample_noise`` (the
        critic loss's sample / its draws) and ``actor_draws`` (``loss_actor``'s noise, noise_bc, t_bc, which, chains) replace
        the draws."""
        m, rp = self.model, self.replay
        loss_c = m.loss_critic(rp, None, None, None, None, self.gamma, inds=inds, next_actions=next_actions,
                               noise=sample_noise).detach()
        self.critic_optimizer.step(m.critic.flat_grads())
        m.critic.mark_updated()
        loss_a = m.loss_actor(rp, self.eta, self.act_steps, inds=inds, **actor_draws).detach()
        if self.itr >= self.n_critic_warmup_itr:
            self.actor_optimizer.step(m.last_loss_grad, max_norm=self.max_grad_norm)
            m.actor.mark_updated()
        m.update_target_critic(self.target_ema_rate)
        return loss_c, loss_a

    def run(self):
        model, dev = self.model, self.device
        S, E = self.n_steps, self.n_envs
        t_start = time.time()
        run_results = []
        cnt_train_step = 0
        last_itr_eval = False
        done_venv = np.zeros(E, dtype=bool)
        prev_obs = None
        metrics = {}
        while self.itr < self.n_train_itr:
            eval_mode = self.itr % self.val_freq == 0 and not self.force_train
            model.eval() if eval_mode else model.train()
            firsts = np.zeros((S + 1, E))
            if self.reset_at_iteration or eval_mode or last_itr_eval or prev_obs is None:
                prev_obs = self.reset_env_all()
                firsts[0] = 1
            else:
                firsts[0] = done_venv
            last_itr_eval = eval_mode
            reward_trajs = np.zeros((S, E))
            # ---------------- rollout (:101-150): the plain sampler on the device, envs on the host
            for step in range(S):
                state = torch.from_numpy(prev_obs["state"]).float().to(dev)
                samples = model(cond={"state": state}, deterministic=eval_mode)
                action = samples.cpu().numpy()[:, :self.act_steps]
                obs, reward, terminated, truncated, info = self.venv.step(action)
                if isinstance(obs, list):
                    obs = {k: np.stack([o[k] for o in obs]) for k in obs[0]}
                done_venv = terminated | truncated
                reward_trajs[step], firsts[step + 1] = reward, done_venv
                if not eval_mode:
                    nxt = obs["state"]
                    for i in np.where(truncated)[0]:  # bootstrap from the pre-reset observation (:133-138)
                        fin = info[i].get("final_obs") if isinstance(info[i], dict) else None
                        if fin is not None:
                            if nxt is obs["state"]:
                                nxt = nxt.copy()
                            nxt[i] = fin["state"] if isinstance(fin, dict) else fin
                    self.replay.append(state, nxt, samples[:, :self.act_steps], reward * self.scale_reward_factor,
                                       terminated.astype(np.float32))
                    cnt_train_step += E * self.act_steps
                prev_obs = obs
            if hasattr(model, "check_sampler_health"):
                model.check_sampler_health()
            avg_ep, avg_best, success = self._episode_stats(firsts, reward_trajs)
            # ---------------- update (:210-260)
            if not eval_mode:
                num_batch = int(S * E / self.batch_size * self.replay_ratio)
                all_inds = self.replay.draw(num_batch, self.batch_size)  # one host draw, one upload
                losses = [self.update_minibatch(all_inds[b]) for b in range(num_batch)]
                if losses:
                    lc, la = (float(x) for x in losses[-1])  # the only device read of the update
                    metrics = {"loss_actor": la, "loss_critic": lc, "actor_lr": self.actor_optimizer.param_groups[0]["lr"],
                               "critic_lr": self.critic_optimizer.param_groups[0]["lr"]}
            # ---------------- schedules, checkpoint, logging (:262-300)
            self.actor_lr_scheduler.step()
            self.critic_lr_scheduler.step()
            if self.itr % self.save_model_freq == 0 or self.itr == self.n_train_itr - 1:
                self.save_model()
            rec = {"itr": self.itr, "step": cnt_train_step}
            if self.itr % self.log_freq == 0:
                rec["time"] = time.time() - t_start
                if eval_mode:
                    rec.update(eval_success_rate=success, eval_episode_reward=avg_ep, eval_best_reward=avg_best)
                    log.info("eval: success rate %8.4f | avg episode reward %8.4f | avg best reward %8.4f", success, avg_ep, avg_best)
                else:
                    rec.update(train_episode_reward=avg_ep, **metrics)
                    log.info("%d: step %8d | loss actor %8.4f | loss critic %8.4f | reward %8.4f | t:%8.4f", self.itr, cnt_train_step,
                             metrics.get("loss_actor", float("nan")), metrics.get("loss_critic", float("nan")), avg_ep, rec["time"])
                if self.use_wandb:
                    self._wandb.log({k: v for k, v in rec.items() if k != "itr"}, step=self.itr)
                run_results.append(rec)
                with open(self.result_path, "wb") as f:
                    pickle.dump(run_results, f)
            self.itr += 1
        return run_results
