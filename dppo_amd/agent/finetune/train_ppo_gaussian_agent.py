"""PPO fine-tuning of a Gaussian policy -- the comparison arm of the DPPO paper.

Mirrors the reference's ``TrainPPOGaussianAgent`` (agent/finetune/train_ppo_gaussian_agent.py:20-400): same cfg keys and
iteration as the diffusion agent, whose ``run()`` and ``_update()`` it inherits; what differs is the sample, ``OneShotSample``
below: one action chunk per step instead of a denoising chain, a scalar log-prob per sample, minibatches over R = n_steps *
n_envs rows.  The minibatch is ``PPO_Gaussian.ppo_update`` (one library call: forward, loss, backward) + fused AdamW; a learned
per-dimension std (``logvar``) is stepped by its own tiny AdamW with the actor's learning rate, like the reference's
``actor_optimizer`` over ``actor_ft.parameters()``.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from dppo_amd import hip
from dppo_amd.agent.finetune.train_ppo_diffusion_agent import TrainPPODiffusionAgent
from dppo_amd.model.diffusion.diffusion import Sample
from dppo_amd.util.optim import FlatAdamW


class _OneShotPolicy:
    """The sampled action chunk is both the trajectory and a one-entry 'chain': what the rollouts (collect_rollout, the pixel
    agents' step loop) call in the model's place."""

    def __init__(self, model):
        self.model, self.horizon_steps = model, model.horizon_steps

    def __call__(self, cond, deterministic=False, return_chain=True):
        a = self.model(cond=cond, deterministic=deterministic)
        return Sample(a, a.reshape(a.shape[0], 1, a.shape[1], a.shape[2]))


class OneShotSample:
    """The sample axis of a PPO agent whose policy draws its action chunk in one shot (Gaussian, GMM); goes in front of the agent
    class that supplies the observation axis."""

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv)
        net = self.model.actor_ft
        self.logvar_optimizer = None
        if getattr(net, "learn_fixed_std", False):
            self.logvar_optimizer = FlatAdamW(net.logvar.data, lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
            self._lv_acc = torch.zeros_like(net.logvar.data)

    def _policy(self):
        return _OneShotPolicy(self.model)

    def _old_logprobs(self, cond, chains):
        return self.model.get_logprobs(cond, chains.reshape(chains.shape[0], -1))[0]

    def _minibatch(self, obs_buf, chains_buf, ret_k, values_buf, adv_k, logp_buf, inds, moments):
        samples = chains_buf.reshape(chains_buf.shape[0], -1)
        return self.model.ppo_update(self._gather(obs_buf, inds), samples[inds], ret_k[inds], values_buf[inds], adv_k[inds],
                                     logp_buf[inds], global_moments=moments)

    def _accumulate_logvar(self, first):
        if self.logvar_optimizer is not None:
            self._lv_acc.copy_(self.model._lv_grad) if first else self._lv_acc.add_(self.model._lv_grad)

    def _logvar_grad(self, accumulated, n_mb, host_entropy):
        """d loss / d logvar behind ``n_mb`` minibatches (``accumulated``: their sum in ``_lv_acc``), all-reduced.  loss = pg +
        entropy_loss * ent_coef + ...: d(-entropy)/d logvar_j = -0.5 / Da inside the clamp range, added here unless the kernel
        did."""
        if self.logvar_optimizer is None:
            return None
        net = self.model.actor_ft
        lv = net.logvar.detach()
        g = (self._lv_acc if accumulated else self.model._lv_grad).clone()
        if self.world > 1:
            dist.all_reduce(g)  # per-rank pg parts are already divided by the GLOBAL count: SUM gives the whole
        if host_entropy:
            g -= n_mb * self.ent_coef * 0.5 / self.action_dim * ((lv >= net.logvar_min) & (lv <= net.logvar_max)).float()
        return g.contiguous()

    def _step_logvar(self, g, max_norm=None, sq_norm=None):
        self.logvar_optimizer.param_groups[0]["lr"] = self.actor_optimizer.param_groups[0]["lr"]
        self.logvar_optimizer.step(g, max_norm=max_norm, sq_norm=sq_norm)

    def _sample_metrics(self, stats):
        ent = stats[hip.GAUSS_STAT_ENTROPY]
        return ent, {"std": stats[hip.GAUSS_STAT_STD], "entropy": ent}


class TrainPPOGaussianAgent(OneShotSample, TrainPPODiffusionAgent):
    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv)
        if getattr(self.model, "entropy_in_kernel", False):  # PPO_GMM: the entropy term's gradient rides the fused backward
            self.model.ent_coef = float(self.ent_coef)
