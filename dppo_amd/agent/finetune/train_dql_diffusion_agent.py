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

from dppo_amd.agent.finetune.train_off_policy_agent import OffPolicyAgent
from dppo_amd.util.optim import FlatAdamW


class TrainDQLDiffusionAgent(OffPolicyAgent):
    nets = ("actor", "critic", "critic_target")

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv, "DQL")
        # ---- TrainDQLDiffusionAgent (:29-81)
        self.n_critic_warmup_itr = cfg.train.n_critic_warmup_itr
        m = self.model
        self.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, cfg.train.actor_lr_scheduler, cfg.train.actor_lr)
        self.critic_lr_scheduler = self._cosine(self.critic_optimizer, cfg.train.critic_lr_scheduler, cfg.train.critic_lr)
        self.replay_ratio = cfg.train.replay_ratio
        self.target_ema_rate = cfg.train.target_ema_rate
        self.eta = cfg.train.eta

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
