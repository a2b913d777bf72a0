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

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.util.optim import FlatAdamW


class TrainIDQLDiffusionAgent(OffPolicyAgent):
    nets = ("actor", "critic_q", "target_q", "critic_v")
    lr_schedulers = ("actor_lr_scheduler", "critic_v_lr_scheduler", "critic_q_lr_scheduler")
    log_line, log_keys = "loss actor %8.4f | reward %8.4f | t:%8.4f", ("loss_actor", "train_episode_reward", "time")

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "IDQL")
        # ---- TrainIDQLDiffusionAgent (:26-96)
        self.n_critic_warmup_itr = cfg.train.n_critic_warmup_itr
        m = self.model
        self.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.critic_q_optimizer = FlatAdamW(m.critic_q.flat_params(), lr=cfg.train.critic_lr,
                                            weight_decay=cfg.train.critic_weight_decay)
        self.critic_v_optimizer = FlatAdamW(m.critic_v.flat_params(), lr=cfg.train.critic_lr,
                                            weight_decay=cfg.train.critic_weight_decay)
        sa, sc = cfg.train.actor_lr_scheduler, cfg.train.critic_lr_scheduler
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, sa, cfg.train.actor_lr)
        self.critic_v_lr_scheduler = self._cosine(self.critic_v_optimizer, sc, cfg.train.critic_lr)
        self.critic_q_lr_scheduler = self._cosine(self.critic_q_optimizer, sc, cfg.train.critic_lr)
        self.use_expectile_exploration = cfg.train.use_expectile_exploration
        self.replay_ratio = cfg.train.replay_ratio
        self.critic_tau = cfg.train.critic_tau
        self.eval_deterministic = cfg.train.get("eval_deterministic", False)
        self.num_sample = cfg.train.eval_sample_num

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

    def _sample(self, state, eval_mode):
        """Best-of-N sampling on the device (reference :139-188)."""
        return self.model(cond={"state": state}, deterministic=eval_mode and self.eval_deterministic, num_sample=self.num_sample,
                          use_expectile_exploration=self.use_expectile_exploration)

    def _metrics(self, lv, lq, la):
        return {"loss_actor": la, "loss_critic": lq + lv, "loss_critic_v": lv, "loss_critic_q": lq,
                "actor_lr": self.actor_optimizer.param_groups[0]["lr"], "critic_lr": self.critic_q_optimizer.param_groups[0]["lr"]}
