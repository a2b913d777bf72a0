"""What the off-policy fine-tuning agents share (IDQL, QSM, DQL, SAC, RLPD, Cal-QL, IBRL) on top of ``TrainAgent`` (set-up, checkpoint,
episode statistics, logging tail): the device-resident replay ring, one env step with its ``final_obs`` bootstrap and ring append,
the iteration of the replay-ratio agents (IDQL, QSM, DQL) as ``run``, and that of the agents which explore at
random first and evaluate by an episode count (SAC, RLPD, Cal-QL) as ``run_by_episode_count``.

A replay-ratio agent supplies its hyper-parameters and optimisers, ``nets`` and ``update_minibatch``; the defaults of
``lr_schedulers``, ``log_line`` / ``log_keys``, ``_sample`` (how an action is drawn) and ``_metrics`` (the logged fields from the
last minibatch's losses) are those of an agent with one actor and one critic optimiser (QSM, DQL).  An episode-count agent
supplies ``update_iteration`` (or its own ``_update``), ``log_alpha``, ``n_explore_steps`` and ``n_eval_episode``; what else differs
between them is the handful of small methods in front of ``run_by_episode_count`` (IBRL, which has no temperature and never acts at
random, overrides ``_train_fields`` and ``explores_at_random``).
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from dppo_amd.agent.finetune.train_agent import TrainAgent
from dppo_amd.util.replay import DeviceReplay
from dppo_amd.util.rollout import stack_obs


class OffPolicyAgent(TrainAgent):
    nets = ()  # the model's networks whose kernel images follow a loaded checkpoint
    replay_cls = DeviceReplay  # the ring's class (Cal-QL's carries each transition's return)
    lr_schedulers = ("actor_lr_scheduler", "critic_lr_scheduler")  # stepped once per iteration, in this order
    # a train iteration's log line after "itr: step |", and the record keys it prints
    log_line = "loss actor %8.4f | loss critic %8.4f | reward %8.4f | t:%8.4f"
    log_keys = ("loss_actor", "loss_critic", "train_episode_reward", "time")

    def __init__(self, cfg, venv, who):
        # the stored action chunk is the critic's action and the actor loss's x_start (reference IDQL :298-301, QSM :236-264);
        # checked before wandb, the env and the model are set up
        assert cfg.act_steps == cfg.horizon_steps, f"{who} needs act_steps == horizon_steps"
        super().__init__(cfg, venv)
        # ---- what every off-policy agent of the reference reads from cfg.train (gamma: applied to the reward of every act_steps
        # env steps)
        self.scale_reward_factor = cfg.train.scale_reward_factor
        self.buffer_size = cfg.train.buffer_size
        self.replay = self.replay_cls(self.buffer_size, self.n_envs, self.n_cond_step * self.obs_dim,
                                   self.act_steps * self.action_dim, self.device)

    def load(self, itr):
        data = torch.load(os.path.join(self.checkpoint_dir, f"state_{itr}.pt"), weights_only=True)
        self.itr = data["itr"]
        self.model.load_state_dict(data["model"])
        for name in self.nets:
            getattr(self.model, name).mark_updated()  # kernel images are rebuilt from the loaded weights on next use

    def env_step(self, state, action, stored, eval_mode):
        """One step of all envs with ``action`` (numpy).  Outside evaluation the transition goes into the ring: ``state`` (the
        device observation the action was drawn at), ``stored`` as its action, the scaled reward, ``terminated``, and the next
        observation -- for a truncated env its pre-reset ``final_obs`` (dict or bare array), so that the bootstrap sees the state
        the episode ended in (reference IDQL :171-177).  The env's own array is copied before the first such write.
        Returns (observation dict, reward, done)."""
        obs, reward, terminated, truncated, info = self.venv.step(action)
        obs = stack_obs(obs)
        if not eval_mode:
            nxt = obs["state"]
            for i in np.where(truncated)[0]:
                fin = info[i].get("final_obs") if isinstance(info[i], dict) else None
                if fin is not None:
                    if nxt is obs["state"]:
                        nxt = nxt.copy()
                    nxt[i] = fin["state"] if isinstance(fin, dict) else fin
            self.replay.append(state, nxt, stored, np.asarray(reward) * self.scale_reward_factor,
                               np.asarray(terminated).astype(np.float32))
        return obs, reward, terminated | truncated

    # ------------------------------------------------------------------------------------------------- IDQL, QSM, DQL
    def _sample(self, state, eval_mode):
        """The action chunk (n_envs, Ta, Da) at the device observations ``state``."""
        return self.model(cond={"state": state}, deterministic=eval_mode)

    def _metrics(self, lc, la):
        """The train record's fields from the last minibatch's losses (host floats, as ``update_minibatch`` returns them)."""
        return {"loss_actor": la, "loss_critic": lc, "actor_lr": self.actor_optimizer.param_groups[0]["lr"],
                "critic_lr": self.critic_optimizer.param_groups[0]["lr"]}

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
            # ---------------- rollout: the sampler on the device, envs on the host
            for step in range(S):
                state = torch.from_numpy(prev_obs["state"]).float().to(dev)
                samples = self._sample(state, eval_mode)
                prev_obs, reward, done_venv = self.env_step(state, samples.cpu().numpy()[:, :self.act_steps],
                                                            samples[:, :self.act_steps], eval_mode)
                reward_trajs[step], firsts[step + 1] = reward, done_venv
                if not eval_mode:
                    cnt_train_step += E * self.act_steps
            if hasattr(model, "check_sampler_health"):
                model.check_sampler_health()
            stats = self._episode_stats(firsts, reward_trajs)
            # ---------------- update
            if not eval_mode:
                num_batch = int(S * E / self.batch_size * self.replay_ratio)
                all_inds = self.replay.draw(num_batch, self.batch_size)  # one host draw, one upload
                losses = [self.update_minibatch(all_inds[b]) for b in range(num_batch)]
                if losses:
                    metrics = self._metrics(*(float(x) for x in losses[-1]))  # the only device read of the update
            # ---------------- schedules, checkpoint, logging
            for name in self.lr_schedulers:
                getattr(self, name).step()
            if self.itr % self.save_model_freq == 0 or self.itr == self.n_train_itr - 1:
                self.save_model()
            if self.itr % self.log_freq == 0:
                self.log_record(run_results, {"itr": self.itr, "step": cnt_train_step}, t_start, eval_mode, stats, metrics)
            self.itr += 1
        return run_results

    # ------------------------------------------------------------------------------------------------- SAC, RLPD, Cal-QL
    # Which of "eval", "update" and "log" wait for ``itr > n_explore_steps``; the others start at ``itr >= n_explore_steps``.  (The
    # reference's agents differ: SAC has ``>`` in all three tests, RLPD in the log line's only, Cal-QL in none.)
    strictly_past_exploration = ("log",)
    explores_at_random = True  # the first ``n_explore_steps`` iterations act at random (IBRL never does: its model always acts)

    def _explore_action(self):
        """Uniformly random actions (reference SAC :121-122): the env's own ``action_space.sample()`` where it has one."""
        space = getattr(self.venv, "action_space", None)
        if space is not None:
            return np.asarray(space.sample(), dtype=np.float32).reshape(self.n_envs, self.act_steps, self.action_dim)
        return np.random.uniform(-1.0, 1.0, size=(self.n_envs, self.act_steps, self.action_dim)).astype(np.float32)

    def _begin_rollout(self, eval_mode):
        """Called once in front of an iteration's rollout; -> the most env steps it may take (an evaluation ends by its episode
        count)."""
        return int(1e5) if eval_mode else self.n_steps

    def _rollout_done(self, eval_mode, cnt_episode):
        """Whether the rollout ends behind a step that brought the finished episodes to ``cnt_episode``."""
        return eval_mode and cnt_episode >= self.n_eval_episode

    def _after_train_step(self, reward, done_venv):
        """Behind every training step's ring append."""

    def _update(self):
        """A training iteration's update past the exploration phase; -> (critic loss, actor loss or None, ...) as device scalars,
        or None where no update was due."""
        return self.update_iteration()

    def _train_fields(self, losses):
        """A logging train iteration's fields from the last update's device scalars: the only device reads of the loop."""
        fields = dict(loss_critic=float(losses[0]), alpha=float(self.log_alpha.detach().exp()))
        if losses[1] is not None:  # (SAC: no actor update yet)
            fields["loss_actor"] = float(losses[1])
        return fields

    def run_by_episode_count(self):
        """The iteration of the agents whose evaluation ends by an episode count (the reference's SAC, RLPD, Cal-QL and IBRL
        agents): rollout, ``_update()``, schedules, checkpoint, record.  With ``explores_at_random`` the first ``n_explore_steps``
        iterations act at random (SAC, RLPD, Cal-QL); IBRL's model acts from iteration 0 and the count only gates evaluation, update
        and log line."""
        model, dev = self.model, self.device
        E = self.n_envs
        X, strict = self.n_explore_steps, self.strictly_past_exploration
        past = lambda what: self.itr > X if what in strict else self.itr >= X
        t_start = time.time()
        run_results = []
        cnt_train_step = 0
        done_venv = np.zeros(E, dtype=bool)
        prev_obs = None
        losses = None
        while self.itr < self.n_train_itr:
            eval_mode = self.itr % self.val_freq == 0 and past("eval") and not self.force_train
            model.eval() if eval_mode else model.train()
            firsts, rewards = [np.zeros(E)], []
            if self.reset_at_iteration or eval_mode or prev_obs is None:
                prev_obs = self.reset_env_all()
                firsts[0] = np.ones(E)
            else:
                firsts[0] = done_venv.astype(np.float64)
            cnt_episode = 0
            # ---------------- rollout
            for step in range(self._begin_rollout(eval_mode)):
                state = torch.from_numpy(prev_obs["state"]).float().to(dev)
                if self.explores_at_random and self.itr < self.n_explore_steps:
                    action = self._explore_action()
                else:
                    action = model(cond={"state": state}, deterministic=eval_mode).cpu().numpy()[:, :self.act_steps]
                prev_obs, reward, done_venv = self.env_step(state, action, action, eval_mode)
                rewards.append(np.asarray(reward, dtype=np.float64))
                firsts.append(done_venv.astype(np.float64))
                if not eval_mode:
                    cnt_train_step += E * self.act_steps
                    self._after_train_step(reward, done_venv)
                cnt_episode += int(np.sum(done_venv))
                if self._rollout_done(eval_mode, cnt_episode):
                    break
            stats = self._episode_stats(np.stack(firsts), np.stack(rewards) if rewards else np.zeros((0, E)))
            # ---------------- update
            if not eval_mode and past("update"):
                new = self._update()
                losses = losses if new is None else new
            # ---------------- schedules, checkpoint, logging
            for name in self.lr_schedulers:
                getattr(self, name).step()
            if self.itr % self.save_model_freq == 0 or self.itr == self.n_train_itr - 1:
                self.save_model()
            rec = {"itr": self.itr, "step": cnt_train_step}
            if self.itr % self.log_freq == 0 and past("log"):
                fields = self._train_fields(losses) if not eval_mode and losses is not None else {}
                self.log_record(run_results, rec, t_start, eval_mode, stats, fields)
            else:
                run_results.append(rec)
            self.itr += 1
        return run_results
