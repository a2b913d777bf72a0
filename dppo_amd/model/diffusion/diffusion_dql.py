"""Diffusion Q-learning.  Mirrors ``dppo/model/diffusion/diffusion_dql.py`` (reference ``DQLDiffusion``): same attribute names
(``actor`` is ``network``, ``critic``, ``critic_target``), so the state dict is the reference's.

The critic's loss is QSM's TD loss word for word (``dppo_qsm_q_loss_fwd_bwd``).  The actor's loss, ``bc + eta * q_loss`` on an
action sampled WITH gradient (``forward_train``, reference :141-179), is ``dppo_dql_actor_fwd_bwd`` (csrc/dql.hip): the persistent
sampler writes the chain with every position kept, the call runs one forward over all of its rows and walks only the gradient
with respect to x back through the K posterior steps (the x0 clamp included); every weight gradient is formed once over all rows.
The flat actor gradient is left in ``last_loss_grad`` like ``DiffusionModel.loss``."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.diffusion.diffusion import DiffusionModel, _FusedDenoiseLoss, flat_views


class DQLDiffusion(DiffusionModel):
    def __init__(self, actor, critic, use_ddim=False, min_sampling_denoising_std=0.1, **kwargs):
        super().__init__(network=actor, use_ddim=use_ddim, **kwargs)
        assert not self.use_ddim, "DQL does not support DDIM"  # (the reference's message: diffusion_dql.py:29)
        if getattr(actor, "is_vision", False):
            raise NotImplementedError("dppo_amd: DQL is built for state observations only (like the reference)")
        if not getattr(critic, "double_q", False):
            raise ValueError("DQL needs the twin critic (double_q=True): the reference's DQLDiffusion unpacks two outputs")
        if self.final_action_clip_value is not None and not self.final_action_clip_value:
            raise ValueError("final_action_clip_value=0 clamps forward() to 0 and forward_train() not at all in the reference: not built")
        self.critic = critic.to(self.device)
        self.critic_target = copy.deepcopy(self.critic)
        self.actor = self.network
        self.min_sampling_denoising_std = min_sampling_denoising_std
        for name in ("_ws_actor", "_ws_q"):
            object.__setattr__(self, name, hip.Workspace())

    def _tables(self, dev):
        """Per device: sqrt(abar), sqrt(1 - abar), and the dppo_step table by diffusion time (entry t: the DDPM coefficients)."""
        cache = self.__dict__.setdefault("_dql_cache", {})
        key = str(dev)
        if key not in cache:
            tab = np.zeros(self.denoising_steps, dtype=hip.STEP_DTYPE)
            for t in range(self.denoising_steps):
                c0, c1, c2, c3, _ = self._ddpm_coefs(t)
                tab[t] = (0, t, -1, 0, c0, c1, c2, c3, 1.0, 0.0)
            cache[key] = (self.sqrt_alphas_cumprod.float().contiguous().to(dev),
                          self.sqrt_one_minus_alphas_cumprod.float().contiguous().to(dev),
                          torch.from_numpy(tab.view(np.uint8)).to(dev))
        return cache[key]

    def _train_cfg(self):
        """forward_train clamps the last x to +-1 whenever final_action_clip_value is truthy (reference :177-178), not to the
        configured value."""
        cfg = DiffusionModel.diffusion_cfg(self)
        if cfg.has_final_clip:
            cfg.final_clip = 1.0
        return cfg

    # ------------------------------------------------------------------ RL training (reference :43-88)
    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, inds=None, next_actions=None, noise=None):
        """mean((q1 - y)^2) + mean((q2 - y)^2), y = r + gamma min(target q1, q2)(s', a') (1 - terminated), a' ~ forward(s') without
        gradient; d loss / d [Q1 | Q2] parameters in ``critic.flat_grads()``, ``last_stats``: {loss, mean q1, mean y}.
        ``next_actions`` / ``noise`` (K+1, N, Ta, Da) replace the sample / its draws."""
        return off_policy.twin_td_loss(self, "DQL", self.critic, self.critic_target, obs, next_obs, actions, rewards, terminated, gamma,
                                       inds, next_actions, noise)

    def loss_actor(self, obs, eta, act_steps, inds=None, noise=None, noise_bc=None, t_bc=None, which=None, chains=None,
                   want_masks=False):
        """bc_loss + eta * q_loss on an action sampled with gradient, and d loss / d actor parameters in ``last_loss_grad``.
        ``obs`` may be a ``DeviceReplay`` (rows ``inds``).  ``which``: 0 is -mean(q1) / mean|q2|, 1 the mirror image; None draws
        the reference's ``np.random.uniform() > 0.5`` (True -> 0).  ``chains`` (N, K+1, Ta, Da): the chain to differentiate
        through, x_K first; None samples it with the persistent sampler (``noise`` (K+1, N, Ta, Da) replaces its draws).
        ``noise_bc`` (N, Ta, Da) / ``t_bc`` (N,) replace the BC term's draws.  ``last_stats``: {loss, bc, q_loss, mean q1, mean q2};
        ``last_d_a`` (N, Ta*Da) = d loss / d action; ``last_chains``; with ``want_masks`` ``last_masks`` (N, K, Ta*Da) bytes."""
        if act_steps != self.horizon_steps:
            raise NotImplementedError(f"dppo_amd: DQL's loss_actor is built for act_steps == horizon_steps (got {act_steps} and "
                                      f"{self.horizon_steps}); every shipped cfg has them equal")
        q, net = self.critic, self.network
        batch, N, keep = off_policy.as_batch("DQL", obs, inds)
        dev = net.flat_params().device
        AF, K = self.horizon_steps * self.action_dim, self.denoising_steps
        if which is None:
            which = 0 if np.random.uniform() > 0.5 else 1
        if chains is None:
            st = off_policy.rows_of("DQL", obs, inds)
            chains = self.forward_train({"state": st.reshape(N, -1)}, noise=noise, return_chain=True).chains
        chains = chains.reshape(N, K + 1, AF).contiguous().float()
        if noise_bc is None:
            noise_bc = torch.randn(N, AF, device=dev)
        if t_bc is None:
            t_bc = torch.randint(0, K, (N,), device=dev)
        noise_bc = noise_bc.reshape(N, AF).contiguous().float()
        t_bc = t_bc.reshape(N).to(torch.int64).contiguous()
        lib, da, dq = hip.load(), net.net_desc(), q.net_desc()
        OD = q.cond_dim
        ws = self._ws_actor.get(lib.dppo_dql_actor_workspace_bytes(C.byref(da), C.byref(dq), self.prec, OD, N, K), dev,
                                "dppo_dql_actor_workspace_bytes")
        k1, k2 = q.packed(self.prec)
        sa, sb, steps = self._tables(dev)
        cfg = self._train_cfg()
        grad = torch.empty_like(net.flat_params())
        stats = torch.empty(hip.DQL_STAT_COUNT, dtype=torch.float64, device=dev)
        d_a = torch.empty(N, AF, dtype=torch.float32, device=dev)
        masks = torch.empty(N, K, AF, dtype=torch.uint8, device=dev) if want_masks else None
        hip.check(lib.dppo_dql_actor_fwd_bwd(
            C.byref(da), C.byref(dq), self.prec, net.flat_params().data_ptr(), net.packed(self.prec, K).data_ptr(),
            q.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2), C.byref(cfg), steps.data_ptr(), K, C.byref(batch), OD, N,
            chains.data_ptr(), noise_bc.data_ptr(), t_bc.data_ptr(), sa.data_ptr(), sb.data_ptr(), float(eta), int(which),
            grad.data_ptr(), stats.data_ptr(), hip.ptr(masks), d_a.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()),
            "dppo_dql_actor_fwd_bwd")
        for name, v in (("last_loss_grad", grad), ("last_stats", stats), ("last_d_a", d_a), ("last_masks", masks),
                        ("last_chains", chains), ("last_which", which)):
            object.__setattr__(self, name, v)
        params = net.trunk_parameters()
        return _FusedDenoiseLoss.apply(stats[0], flat_views(grad, params), *params)

    def update_target_critic(self, tau):
        off_policy.polyak(self.critic_target, self.critic, tau)

    # ------------------------------------------------------------------ sampling (reference :100-179)
    @torch.no_grad()
    def forward(self, cond, deterministic=False, noise=None):
        """The plain K-step sampler: std clipped at ``min_sampling_denoising_std``, or (deterministic) 0 at t = 0 and 1e-3
        above.  ``noise`` (K+1, B, Ta, Da) replaces the in-kernel draws.  Returns (B, Ta, Da)."""
        if "rgb" in cond:
            raise NotImplementedError("dppo_amd: DQL is built for state observations only (like the reference)")
        return self._run_sampler(cond, bool(deterministic), False, False, noise, None, "DQLDiffusion.forward").trajectories

    @torch.no_grad()
    def forward_train(self, cond, deterministic=False, noise=None, return_chain=False):
        """The reference's differentiable sampler (:141-179) as far as its VALUE goes: the same chain as ``forward`` except that
        the last x is clamped to +-1 whenever ``final_action_clip_value`` is truthy.  Returns the sample (B, Ta, Da) -- the
        gradient through it is ``loss_actor``'s business -- or, with ``return_chain``, ``Sample(trajectories, chains)`` with
        every chain position kept (B, K+1, Ta, Da), x_K first."""
        if "rgb" in cond:
            raise NotImplementedError("dppo_amd: DQL is built for state observations only (like the reference)")
        real_ft = self.ft_denoising_steps
        try:  # every position kept: the sampler's chain geometry with all K steps marked as recorded
            object.__setattr__(self, "diffusion_cfg", self._train_cfg)
            self.ft_denoising_steps = self.denoising_steps
            smp = self._run_sampler(cond, bool(deterministic), True, False, noise, None, "DQLDiffusion.forward_train")
        finally:
            object.__delattr__(self, "diffusion_cfg")
            self.ft_denoising_steps = real_ft
        return smp if return_chain else smp.trajectories
