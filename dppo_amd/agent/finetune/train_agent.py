"""What every fine-tuning agent shares.  Mirrors the reference's ``TrainAgent`` (agent/finetune/train_agent.py:19-145): seeding,
wandb, the vectorised env and its seeds, the dimensions, the ``cfg.train`` / ``cfg.env`` keys both families read, the log and
checkpoint paths, ``reset_env_all``, ``save_model``, the episode statistics and a logging iteration's tail.  The PPO agents
(train_ppo_diffusion_agent.py) and the off-policy agents (train_off_policy_agent.py) derive from it.

The class knows its rank: with ``torch.distributed`` initialised every rank owns a shard of the envs (seeds ``seed + rank * n_envs
+ i``), and rank 0 alone talks to wandb, makes the directories and writes checkpoints.  One process is rank 0 of 1.
"""
from __future__ import annotations

import logging
import os
import pickle
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from dppo_amd.cfg.loader import instantiate
from dppo_amd.env.synthetic import make_venv
from dppo_amd.util.rollout import stack_obs
from dppo_amd.util.scheduler import CosineAnnealingWarmupRestarts

log = logging.getLogger(__name__)


def episode_stats(firsts, reward_trajs, act_steps, success_threshold, best_is_sum=False):
    """(average episode reward, average best reward, success rate, episode count) over the episodes that start and end within
    the window (reference :190-225).  An episode's best reward is its largest per-env-step reward, or with ``best_is_sum`` (the
    evaluation of furniture's sparse reward) its sum."""
    ep_rewards, ep_best = [], []
    for e in range(firsts.shape[1]):
        starts = np.where(firsts[:, e] == 1)[0]
        for i in range(len(starts) - 1):
            a, b = starts[i], starts[i + 1]
            if b - a > 1:
                seg = reward_trajs[a:b, e]
                ep_rewards.append(seg.sum())
                ep_best.append(seg.sum() if best_is_sum else seg.max() / act_steps)
    n_ep = len(ep_rewards)
    avg_ep = float(np.mean(ep_rewards)) if n_ep else 0.0
    avg_best = float(np.mean(ep_best)) if n_ep else 0.0
    success = float(np.mean(np.array(ep_best) >= success_threshold)) if n_ep else 0.0
    return avg_ep, avg_best, success, n_ep


class TrainAgent:
    # log_line, log_keys: a train iteration's log line after "itr: step |" and the record keys it prints (each family's own)

    def __init__(self, cfg, venv=None):
        self.cfg = cfg
        self.device = cfg.device
        self.seed = cfg.get("seed", 42)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        random.seed(self.seed)
        np.random.seed(self.seed)
        torch.manual_seed(self.seed)  # identical on every rank -> identical initial weights

        self.use_wandb = cfg.get("wandb", None) is not None and self.rank == 0
        if self.use_wandb:
            try:
                import wandb
                wandb.init(entity=cfg.wandb.entity, project=cfg.wandb.project, name=cfg.wandb.run, config=dict(cfg))
                self._wandb = wandb
            except ImportError:
                log.warning("wandb is not installed; logging to the python logger and result.pkl only")
                self.use_wandb = False
        self.n_envs = cfg.env.n_envs  # per rank: env shards are independent
        self.venv = venv if venv is not None else make_venv(cfg)
        if hasattr(self.venv, "seed") and cfg.env.get("env_type", None) != "furniture":
            self.venv.seed([self.seed + self.rank * self.n_envs + i for i in range(self.n_envs)])
        self.n_cond_step, self.obs_dim, self.action_dim = cfg.cond_steps, cfg.obs_dim, cfg.action_dim
        self.act_steps, self.horizon_steps = cfg.act_steps, cfg.horizon_steps
        self.max_episode_steps = cfg.env.get("max_episode_steps", 1000)
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
        if self.rank == 0:
            os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.log_freq = cfg.train.get("log_freq", 1)
        self.save_model_freq = cfg.train.save_model_freq
        self.gamma = cfg.train.gamma

    @staticmethod
    def _cosine(opt, sched_cfg, lr):
        return CosineAnnealingWarmupRestarts(opt, first_cycle_steps=sched_cfg.first_cycle_steps, cycle_mult=1.0, max_lr=lr,
                                             min_lr=sched_cfg.min_lr, warmup_steps=sched_cfg.warmup_steps, gamma=1.0)

    def reset_env_all(self, options_venv=None):
        return stack_obs(self.venv.reset_arg(options_list=options_venv or [{} for _ in range(self.n_envs)]))

    def save_model(self):
        """checkpoint/state_{itr}.pt = {"itr", "model": state_dict} (train_agent.py:125-135)."""
        if self.rank != 0:
            return
        path = os.path.join(self.checkpoint_dir, f"state_{self.itr}.pt")
        torch.save({"itr": self.itr, "model": self.model.state_dict()}, path)
        log.info("Saved model to %s", path)

    def _episode_stats(self, firsts, reward_trajs):
        """(average episode reward, average best reward, success rate) over the episodes that finish within the iteration."""
        return episode_stats(firsts, reward_trajs, self.act_steps, self.best_reward_threshold_for_success)[:3]

    def log_record(self, run_results, rec, t_start, eval_mode, stats, train_fields):
        """A logging iteration's tail: ``time`` and the evaluation's or the training's fields into ``rec``, the log line, wandb,
        ``rec`` onto ``run_results`` and all of it into result.pkl."""
        avg_ep, avg_best, success = stats
        rec["time"] = time.time() - t_start
        if eval_mode:
            rec.update(eval_success_rate=success, eval_episode_reward=avg_ep, eval_best_reward=avg_best)
            log.info("eval: success rate %8.4f | avg episode reward %8.4f | avg best reward %8.4f", success, avg_ep, avg_best)
        else:
            rec.update(train_episode_reward=avg_ep, **train_fields)
            log.info("%d: step %8d | " + self.log_line, rec["itr"], rec["step"], *[rec.get(k, float("nan")) for k in self.log_keys])
        if self.use_wandb:
            self._wandb.log({k: v for k, v in rec.items() if k != "itr"}, step=self.itr)
        run_results.append(rec)
        with open(self.result_path, "wb") as f:
            pickle.dump(run_results, f)
