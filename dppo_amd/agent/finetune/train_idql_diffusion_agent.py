"""IDQL fine-tuning agent.

Mirrors the reference's ``TrainIDQLDiffusionAgent`` (agent/finetune/train_idql_diffusion_agent.py:24-367): same cfg keys, same
iteration structure (rollout with best-of-N action selection -> FIFO replay -> ``n_steps * n_envs / batch_size * replay_ratio``
minibatch updates of V, Q, the Polyak target and the actor, in that order -> LR schedules -> checkpoint), same checkpoint
format.  What changed is WHERE things live: the replay buffer is a device-resident ring (dppo_amd/util/replay.py) instead of
five host deques copied to numpy, flattened and uploaded five arrays at a time per minibatch (:233-270); the minibatch indices
of a whole iteration are drawn on the host once and uploaded once; every loss, gradient, optimiser step and the Polyak average
is a library call, and nothing in the minibatch loop reads the device (the losses for logging are read once after it).
State observations only, like the reference.
"""
from __future__ import annotations

import logging
import os
import pickle
import random
import time

import numpy as np
import torch

from dppo_amd.cfg.loader import instantiate
from dppo_amd.env.synthetic import make_venv
from dppo_amd.util.optim import FlatAdamW
from dppo_amd.util.replay import DeviceReplay
from dppo_amd.util.scheduler import CosineAnnealingWarmupRestarts

log = logging.getLogger(__name__)


class OffPolicyDiffusionAgent:
    """What the off-policy fine-tuning agents share (IDQL here, QSM in train_qsm_diffusion_agent.py): the reference's
    ``TrainAgent`` set-up, the env reset, the checkpoint and the per-iteration episode statistics."""

    def _init_train_agent(self, cfg, venv, who):
        self.cfg = cfg
        self.device = cfg.device
        self.seed = cfg.get("seed", 42)
        random.seed(self.seed)
        np.random.seed(self.seed)
        torch.manual_seed(self.seed)

        # ---- TrainAgent (train_agent.py:21-120)
        self.use_wandb = cfg.get("wandb", None) is not None
        if self.use_wandb:
            try:
                import wandb
                wandb.init(entity=cfg.wandb.entity, project=cfg.wandb.project, name=cfg.wandb.run, config=dict(cfg))
                self._wandb = wandb
            except ImportError:
                log.warning("wandb is not installed; logging to the python logger and result.pkl only")
                self.use_wandb = False
        self.n_envs = cfg.env.n_envs
        self.venv = venv if venv is not None else make_venv(cfg)
        if hasattr(self.venv, "seed") and cfg.env.get("env_type", None) != "furniture":
            self.venv.seed([self.seed + i for i in range(self.n_envs)])
        self.n_cond_step, self.obs_dim, self.action_dim = cfg.cond_steps, cfg.obs_dim, cfg.action_dim
        self.act_steps, self.horizon_steps = cfg.act_steps, cfg.horizon_steps
        # the stored action chunk is the actor loss's x_start (reference :298-301)
        assert self.act_steps == self.horizon_steps, f"{who} needs act_steps == horizon_steps"
        self.reset_at_iteration = cfg.env.get("reset_at_iteration", True)
        self.batch_size = cfg.train.batch_size
        self.model = instantiate(cfg.model)
        self.itr = 0
        self.n_train_itr, self.val_freq = cfg.train.n_train_itr, cfg.train.val_freq
        self.force_train = cfg.train.get("force_train", False)
        self.n_steps = cfg.train.n_steps
        self.best_reward_threshold_for_success = cfg.env.get("best_reward_threshold_for_success", 0)
        self.max_grad_norm = cfg.train.get("max_grad_norm", None)
        self.logdir = cfg.logdir
        self.checkpoint_dir = os.path.join(self.logdir, "checkpoint")
        self.result_path = os.path.join(self.logdir, "result.pkl")
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.log_freq = cfg.train.get("log_freq", 1)
        self.save_model_freq = cfg.train.save_model_freq

    def reset_env_all(self, options_venv=None):
        obs = self.venv.reset_arg(options_list=options_venv or [{} for _ in range(self.n_envs)])
        if isinstance(obs, list):
            obs = {k: np.stack([o[k] for o in obs]) for k in obs[0]}
        return obs

    def save_model(self):
        """checkpoint/state_{itr}.pt = {"itr", "model": state_dict} (train_agent.py:125-135)."""
        path = os.path.join(self.checkpoint_dir, f"state_{self.itr}.pt")
        torch.save({"itr": self.itr, "model": self.model.state_dict()}, path)
        log.info("Saved model to %s", path)

    def _episode_stats(self, firsts, reward_trajs):
        """(average episode reward, average best reward, success rate) over the episodes that finish within the iteration
        (reference :190-225)."""
        ep_rewards, ep_best = [], []
        for e in range(self.n_envs):
            starts = np.where(firsts[:, e] == 1)[0]
            for i in range(len(starts) - 1):
                a, b = starts[i], starts[i + 1]
                if b - a > 1:
                    seg = reward_trajs[a:b, e]
                    ep_rewards.append(seg.sum())
                    ep_best.append(seg.max() / self.act_steps)
        n_ep = len(ep_rewards)
        avg_ep = float(np.mean(ep_rewards)) if n_ep else 0.0
        avg_best = float(np.mean(ep_best)) if n_ep else 0.0
        success = float(np.mean(np.array(ep_best) >= self.best_reward_threshold_for_success)) if n_ep else 0.0
        return avg_ep, avg_best, success


class TrainIDQLDiffusionAgent(OffPolicyDiffusionAgent):
    def __init__(self, cfg, venv=None):
        self._init_train_agent(cfg, venv, "IDQL")
        # ---- TrainIDQLDiffusionAgent (:26-96)
        self.gamma = cfg.train.gamma  # applied to the reward of every act_steps env steps
        self.n_critic_warmup_itr = cfg.train.n_critic_warmup_itr
        m = self.model
        self.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.critic_q_optimizer = FlatAdamW(m.critic_q.flat_params(), lr=cfg.train.critic_lr,
                                            weight_decay=cfg.train.critic_weight_decay)
        self.critic_v_optimizer = FlatAdamW(m.critic_v.flat_params(), lr=cfg.train.critic_lr,
                                            weight_decay=cfg.train.critic_weight_decay)
        sa, sc = cfg.train.actor_lr_scheduler, cfg.train.critic_lr_scheduler
        mk = lambda opt, s, lr: CosineAnnealingWarmupRestarts(opt, first_cycle_steps=s.first_cycle_steps, cycle_mult=1.0, max_lr=lr,
                                                              min_lr=s.min_lr, warmup_steps=s.warmup_steps, gamma=1.0)
        self.actor_lr_scheduler = mk(self.actor_optimizer, sa, cfg.train.actor_lr)
        self.critic_v_lr_scheduler = mk(self.critic_v_optimizer, sc, cfg.train.critic_lr)
        self.critic_q_lr_scheduler = mk(self.critic_q_optimizer, sc, cfg.train.critic_lr)
        self.buffer_size = cfg.train.buffer_size
        self.use_expectile_exploration = cfg.train.use_expectile_exploration
        self.scale_reward_factor = cfg.train.scale_reward_factor
        self.replay_ratio = cfg.train.replay_ratio
        self.critic_tau = cfg.train.critic_tau
        self.eval_deterministic = cfg.train.get("eval_deterministic", False)
        self.num_sample = cfg.train.eval_sample_num
        self.replay = DeviceReplay(self.buffer_size, self.n_envs, self.n_cond_step * self.obs_dim,
                                   self.act_steps * self.action_dim, self.device)

    def load(self, itr):
        data = torch.load(os.path.join(self.checkpoint_dir, f"state_{itr}.pt"), weights_only=True)
        self.itr = data["itr"]
        self.model.load_state_dict(data["model"])
        for net in (self.model.actor, self.model.critic_q, self.model.target_q, self.model.critic_v):
            net.mark_updated()  # kernel images are rebuilt from the loaded weights on next use

    # -------------------------------------------------------------------------------------------------
    def update_minibatch(self, inds, noise=None, t=None):
        """One minibatch in the reference's order (:272-309): V loss and step; Q loss with the UPDATED V and step; Polyak and
        re-pack; actor MSE, stepped only after the critic warm-up.  Nothing here reads the device.  Returns the three losses
        as device scalars."""
        m, rp = self.model, self.replay
        loss_v = m.loss_critic_v(rp, None, inds=inds).detach()
        self.critic_v_optimizer.step(m.critic_v.flat_grads())
        m.critic_v.mark_updated()
        loss_q = m.loss_critic_q(rp, None, None, None, None, self.gamma, inds=inds).detach()
        self.critic_q_optimizer.step(m.critic_q.flat_grads())
        m.critic_q.mark_updated()
        m.update_target_critic(self.critic_tau)
        m.target_q.packed(m.prec)
        obs_b, _, act_b, _, _ = rp.gather(inds)
        N = inds.numel()
        loss_a = m.loss(act_b.view(N, self.horizon_steps, self.action_dim), {"state": obs_b.view(N, self.n_cond_step, self.obs_dim)},
                        noise=noise, t=t).detach()
        if self.itr >= self.n_critic_warmup_itr:
            self.actor_optimizer.step(m.last_loss_grad, max_norm=self.max_grad_norm)
            m.actor.mark_updated()
        return loss_v, loss_q, loss_a

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
            # ---------------- rollout (:139-188): best-of-N sampling on the device, envs on the host
            for step in range(S):
                state = torch.from_numpy(prev_obs["state"]).float().to(dev)
                samples = model(cond={"state": state}, deterministic=eval_mode and self.eval_deterministic,
                                num_sample=self.num_sample, use_expectile_exploration=self.use_expectile_exploration)
                action = samples.cpu().numpy()[:, :self.act_steps]
                obs, reward, terminated, truncated, info = self.venv.step(action)
                if isinstance(obs, list):
                    obs = {k: np.stack([o[k] for o in obs]) for k in obs[0]}
                done_venv = terminated | truncated
                reward_trajs[step], firsts[step + 1] = reward, done_venv
                if not eval_mode:
                    nxt = obs["state"]
                    for i in np.where(truncated)[0]:  # bootstrap from the pre-reset observation (:171-177)
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
            # ---------------- episode statistics (:190-225)
            avg_ep, avg_best, success = self._episode_stats(firsts, reward_trajs)
            # ---------------- update (:227-309)
            if not eval_mode:
                num_batch = int(S * E / self.batch_size * self.replay_ratio)
                all_inds = self.replay.draw(num_batch, self.batch_size)  # one host draw, one upload
                losses = [self.update_minibatch(all_inds[b]) for b in range(num_batch)]
                if losses:
                    lv, lq, la = (float(x) for x in losses[-1])  # the only device read of the update
                    metrics = {"loss_actor": la, "loss_critic": lq + lv, "loss_critic_v": lv, "loss_critic_q": lq,
                               "actor_lr": self.actor_optimizer.param_groups[0]["lr"],
                               "critic_lr": self.critic_q_optimizer.param_groups[0]["lr"]}
            # ---------------- schedules, checkpoint, logging (:311-367)
            self.actor_lr_scheduler.step()
            self.critic_v_lr_scheduler.step()
            self.critic_q_lr_scheduler.step()
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
                    log.info("%d: step %8d | loss actor %8.4f | reward %8.4f | t:%8.4f", self.itr, cnt_train_step,
                             metrics.get("loss_actor", float("nan")), avg_ep, rec["time"])
                if self.use_wandb:
                    self._wandb.log({k: v for k, v in rec.items() if k != "itr"}, step=self.itr)
                run_results.append(rec)
                with open(self.result_path, "wb") as f:
                    pickle.dump(run_results, f)
            self.itr += 1
        return run_results
