"""Cal-QL agent.

Mirrors the reference's ``TrainCalQLAgent`` (agent/finetune/train_calql_agent.py:22-503): same cfg keys in the same order, one env,
and its two modes.  Offline (``train_online: false``): no training rollouts, ``num_update`` updates per iteration on ``batch_size``
offline rows.  Online: a rollout until ``n_episode_per_epoch`` episodes end (uniformly random actions while ``itr <
n_explore_steps``), as many updates as the first episode finished in the iteration had steps, each on ``batch_size // 2`` offline
rows followed by as many online ones.  Evaluation by episode count every ``val_freq`` iterations from ``n_explore_steps`` on.  Both
cosine schedules are stepped every iteration; same checkpoint format.

The offline dataset (with its Monte-Carlo returns) and the replay ring (``ReturnsReplay``: a sixth column with the reward-to-go,
written when an episode closes) are device-resident; a batch is two gathers and one concatenation on the device.  Every loss,
gradient, optimiser step and the Polyak average is a library call; the random actions of the conservative term are drawn inside the
critic's kernel; the temperature's snapshot is a device scalar where the reference reads it back with ``.item()``: nothing in
``update_iteration`` reads the device, and losses are read on logging iterations only.  ``log_alpha`` is a device float64 tensor
stepped by ``torch.optim.Adam``.  State observations only.

Deviations from the reference:
  1. it also appends EVALUATION episodes' returns to ``reward_to_go_buffer``, which misaligns returns and transitions; here only
     training episodes are stored;
  2. it leaves one-step episodes out of the returns (``end - start > 1``) but keeps their transitions; here every closed episode gets
     its returns;
  3. if no episode finished in a training iteration it reads an unbound or stale ``reward_trajs_split``; here that iteration makes no
     update;
  4. (imitated, not a deviation in behaviour) online returns are computed from the UNSCALED rewards while rewards are stored scaled;
     every shipped cfg has ``scale_reward_factor: 1.0``.
"""
from __future__ import annotations

import numpy as np
import torch

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.cfg.loader import instantiate
from dppo_amd.util.optim import FlatAdamW
from dppo_amd.util.replay import ReturnsReplay


def discounted_returns(rewards, gamma):
    """returns[t] = rewards[t] + gamma returns[t + 1] (reference :258-270), in float64 on the host."""
    out, prev = np.zeros(len(rewards), dtype=np.float64), 0.0
    for t in range(len(rewards) - 1, -1, -1):
        prev = out[t] = float(rewards[t]) + gamma * prev
    return out


class TrainCalQLAgent(OffPolicyAgent):
    nets = ("network", "critic", "target_critic")
    log_line = "loss actor %8.4f | loss critic %8.4f | reward %8.4f | alpha %8.4f | t %8.4f"
    log_keys = ("loss_actor", "loss_critic", "train_episode_reward", "alpha", "time")
    replay_cls = ReturnsReplay  # a sixth column: the reward-to-go, written when an episode closes
    strictly_past_exploration = ()

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "Cal-QL")
        assert self.n_envs == 1, "Cal-QL only supports single env for now"
        # ---- TrainCalQLAgent (:23-101), in its order
        self.train_online = cfg.train.train_online
        self.dataset_offline = instantiate(cfg.offline_dataset)
        m = self.model
        self.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, cfg.train.actor_lr_scheduler, cfg.train.actor_lr)
        self.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        self.critic_lr_scheduler = self._cosine(self.critic_optimizer, cfg.train.critic_lr_scheduler, cfg.train.critic_lr)
        self.target_ema_rate = cfg.train.target_ema_rate
        self.n_random_actions = m.n_random_actions = cfg.train.n_random_actions
        self.num_update = cfg.train.num_update
        if self.train_online:
            self.n_episode_per_epoch = cfg.train.n_episode_per_epoch
        self.n_eval_episode = cfg.train.n_eval_episode
        self.n_explore_steps = cfg.train.n_explore_steps
        self.log_alpha = torch.tensor(np.log(cfg.train.init_temperature), dtype=torch.float64, device=self.device,
                                      requires_grad=True)
        self.automatic_entropy_tuning = cfg.train.automatic_entropy_tuning
        self.target_entropy = cfg.train.target_entropy
        self.log_alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=cfg.train.critic_lr)

    # -------------------------------------------------------------------------------------------------
    def draw_batch(self):
        """One batch (:318-392): offline rows (``batch_size // 2`` online, ``batch_size`` offline), then in online mode as many rows
        of closed episodes from the replay ring, both drawn with replacement from the global numpy generator in that order,
        gathered and concatenated on the device, the returns with them."""
        dev = self.device
        n_off = self.batch_size // 2 if self.train_online else self.batch_size
        off_i = np.random.choice(len(self.dataset_offline), n_off)
        off = self.dataset_offline.gather(torch.from_numpy(off_i.astype(np.int64)).to(dev))
        flat = lambda x, n: x.reshape(n, -1).float()
        col = lambda x, n: x.reshape(n).float()
        b = dict(obs=flat(off.conditions["state"], n_off), next_obs=flat(off.conditions["next_state"], n_off),
                 actions=flat(off.actions, n_off), reward=col(off.rewards, n_off), terminated=col(off.dones, n_off),
                 returns=col(off.reward_to_gos, n_off))
        if self.train_online:
            n_on = self.batch_size // 2
            ok = self.replay.closed_indices()
            on_i = ok[np.random.choice(len(ok), n_on)]
            on = self.replay.gather(torch.from_numpy(on_i.astype(np.int64)).to(dev))
            for k, x in zip(("obs", "next_obs", "actions"), on[:3]):
                b[k] = torch.cat([b[k], flat(x, n_on)], dim=0)
            for k, x in zip(("reward", "terminated", "returns"), on[3:]):
                b[k] = torch.cat([b[k], col(x, n_on)], dim=0)
        return b

    def update_iteration(self, batches=None, samples=None, sample_noise=None, random_actions=None, actor_noise=None, temp_noise=None):
        """ONE update in the reference's order (:408-445): the temperature's snapshot; the critic loss (its random actions drawn in
        the kernel), the critic's step, Polyak; the actor loss on the same batch with the snapshot and its step; with
        ``automatic_entropy_tuning`` the temperature loss and its step.  Nothing here reads the device.  Returns (critic loss, actor
        loss, temperature loss or None) as device scalars.  ``batches`` (the batch, or a sequence whose first entry it is),
        ``samples`` / ``sample_noise`` (the critic loss's policy samples / their draws), ``random_actions``, ``actor_noise`` and
        ``temp_noise`` replace the draws."""
        m = self.model
        b = self.draw_batch() if batches is None else (batches if isinstance(batches, dict) else batches[0])
        alpha = self.log_alpha.detach().exp()
        loss_c = m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], random_actions, b["reward"], b["returns"],
                               b["terminated"], self.gamma, samples=samples, noise=sample_noise).detach()
        self.critic_optimizer.step(m.critic.flat_grads())
        m.critic.mark_updated()
        m.update_target_critic(self.target_ema_rate)
        loss_a = m.loss_actor({"state": b["obs"]}, alpha, noise=actor_noise).detach()
        self.actor_optimizer.step(m.last_loss_grad)
        m.network.mark_updated()
        loss_t = None
        if self.automatic_entropy_tuning:
            self.log_alpha_optimizer.zero_grad()
            lt = m.loss_temperature({"state": b["obs"]}, self.log_alpha, self.target_entropy, noise=temp_noise)
            lt.backward()
            self.log_alpha_optimizer.step()
            loss_t = lt.detach()
        return loss_c, loss_a, loss_t

    # ------------------------------------------------------------------------------------------------- the loop's Cal-QL parts
    def _begin_rollout(self, eval_mode):
        """An evaluation and an online rollout end by their episode count; offline training does not step the env (:160-165)."""
        self._first_episode_steps = None  # of the first training episode that finishes in this iteration
        return int(1e5) if eval_mode or self.train_online else 0

    def _rollout_done(self, eval_mode, cnt_episode):
        return cnt_episode >= (self.n_eval_episode if eval_mode else self.n_episode_per_epoch)

    def _after_train_step(self, reward, done_venv):
        """The open episode's UNSCALED rewards (deviation 4); when it closes, its returns go into its own transitions' slots."""
        self._open_rewards.append(float(np.asarray(reward).reshape(-1)[0]))
        if done_venv[0]:
            self.replay.close_episode(discounted_returns(self._open_rewards, self.gamma))
            if self._first_episode_steps is None:
                self._first_episode_steps = len(self._open_rewards)
            self._open_rewards = []

    def _update(self):
        """(:301-445) online as many updates as the first episode finished in the iteration had steps, offline ``num_update``."""
        losses = None
        for _ in range((self._first_episode_steps or 0) if self.train_online else self.num_update):
            losses = self.update_iteration()
        return losses

    def run(self):
        self._open_rewards = []  # of the open training episode, which may span iterations: its returns are formed when it closes
        return self.run_by_episode_count()
