"""Q-score matching.  Mirrors ``dppo/model/diffusion/diffusion_qsm.py`` (reference ``QSMDiffusion``) on top of
``RWRDiffusion``'s sampling schedule (``diffusion_rwr.py:65-103``: std clipped at ``min_sampling_denoising_std``, which is
``DiffusionModel._sampling_schedule`` with no fine-tuned steps).

The actor's loss is ``mse(-eps_theta(x_t, t, s), c * g)`` with ``g = mean(dQ1/da, dQ2/da)`` at ``(s, x_t)``; negation is exact,
so it is ``mse(eps_theta(x_t, t, s), -c * g)``: the denoising MSE with another regression target.  ``dppo_qsm_actor_target``
(csrc/qsm.hip) gathers the minibatch, draws nothing, forms ``x_t`` and ``-c * g`` and writes them where
``DiffusionModel._mse_on_pairs`` reads its operands; no parameter gradient of the critic is computed on the way.  The critic's
TD loss bootstraps from the target twin at ``(s', a' ~ pi(s'))`` and leaves its flat gradient in ``critic_q.flat_grads()``."""
from __future__ import annotations

import copy
import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.diffusion.diffusion import DiffusionModel


class QSMDiffusion(DiffusionModel):
    def __init__(self, actor, critic, min_sampling_denoising_std=0.1, use_ddim=False, **kwargs):
        super().__init__(network=actor, use_ddim=use_ddim, **kwargs)
        assert not self.use_ddim, "RWR does not support DDIM"  # (the reference's message: diffusion_rwr.py:27)
        if getattr(actor, "is_vision", False):
            raise NotImplementedError("dppo_amd: QSM is built for state observations only (like the reference)")
        if not getattr(critic, "double_q", False):
            raise ValueError("QSM needs the twin critic (double_q=True): the reference's QSMDiffusion unpacks two outputs")
        self.min_sampling_denoising_std = min_sampling_denoising_std
        self.critic_q = critic.to(self.device)
        self.target_q = copy.deepcopy(critic).to(self.device)
        self.actor = self.network
        object.__setattr__(self, "_ws_target", hip.Workspace())
        object.__setattr__(self, "_ws_q", hip.Workspace())

    def _tables(self, dev):
        """sqrt(abar), sqrt(1 - abar) on the device (the schedule is fixed after construction; one pair per device)."""
        cache = self.__dict__.setdefault("_qsample_cache", {})
        key = str(dev)
        if key not in cache:
            cache[key] = (self.sqrt_alphas_cumprod.float().contiguous().to(dev),
                          self.sqrt_one_minus_alphas_cumprod.float().contiguous().to(dev))
        return cache[key]

    # ------------------------------------------------------------------ RL training (reference :36-95)
    def loss_actor(self, obs, actions, q_grad_coeff, inds=None, noise=None, t=None, want_grad=False):
        """mse(eps_theta(x_t, t, s), -q_grad_coeff * g), g the twin's mean action gradient at (s, x_t) with the critic as it
        stands.  ``obs`` may be a ``DeviceReplay`` (rows ``inds``).  ``noise`` (N, Ta, Da) / ``t`` (N,) replace the draws
        (parity runs).  The flat actor gradient is left in ``last_loss_grad`` like ``DiffusionModel.loss``; ``want_grad``:
        g (N, Ta*Da) in ``last_q_grad``."""
        q = self.critic_q
        batch, N, keep = off_policy.as_batch("QSM", obs, inds, actions)
        dev = q.flat_params().device
        AF, K = self.horizon_steps * self.action_dim, self.denoising_steps
        if noise is None:
            noise = torch.randn(N, AF, device=dev)
        if t is None:
            t = torch.randint(0, K, (N,), device=dev)  # below denoising_steps: no range check (a device read) needed
        elif t.numel() and int(t.max()) >= K:
            raise ValueError(f"t must lie below denoising_steps={K}")
        noise = noise.reshape(N, AF).contiguous().float()
        t = t.reshape(N).to(torch.int64).contiguous()
        lib, dq = hip.load(), q.net_desc()
        OD = q.cond_dim
        ws = self._ws_target.get(lib.dppo_qsm_actor_target_workspace_bytes(C.byref(dq), self.prec, OD, N), dev,
                                 "dppo_qsm_actor_target_workspace_bytes")
        k1, k2 = q.packed(self.prec)
        sa, sb = self._tables(dev)
        pairs = torch.empty(N, 2, AF, dtype=torch.float32, device=dev)
        obs_out = torch.empty(N, OD, dtype=torch.float32, device=dev)
        g = torch.empty(N, AF, dtype=torch.float32, device=dev) if want_grad else None
        hip.check(lib.dppo_qsm_actor_target(
            C.byref(dq), self.prec, q.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2), C.byref(batch), OD, N, noise.data_ptr(),
            t.data_ptr(), sa.data_ptr(), sb.data_ptr(), K, float(q_grad_coeff), pairs.data_ptr(), obs_out.data_ptr(), hip.ptr(g),
            ws.data_ptr(), ws.numel(), hip.stream()), "dppo_qsm_actor_target")
        object.__setattr__(self, "last_q_grad", g)
        object.__setattr__(self, "last_pairs", pairs)
        return self._mse_on_pairs(pairs, t, obs_out, N)

    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, inds=None, next_actions=None, noise=None):
        """mean((q1 - y)^2) + mean((q2 - y)^2), y = r + gamma min(target q1, q2)(s', a') (1 - terminated); d loss / d [Q1 | Q2]
        parameters in ``critic_q.flat_grads()``, ``last_stats``: {loss, mean q1, mean y}.  ``next_actions`` None: a' is sampled
        with ``forward`` at the gathered next observations (``noise`` (K+1, N, Ta, Da) replaces its draws)."""
        return off_policy.twin_td_loss(self, "QSM", self.critic_q, self.target_q, obs, next_obs, actions, rewards, terminated, gamma,
                                       inds, next_actions, noise)

    def update_target_critic(self, tau):
        off_policy.polyak(self.target_q, self.critic_q, tau)

    # ------------------------------------------------------------------ sampling (reference diffusion_rwr.py:65-103)
    @torch.no_grad()
    def forward(self, cond, deterministic=False, noise=None):
        """The plain K-step sampler: std clipped at ``min_sampling_denoising_std``, or (deterministic) 0 at t = 0 and 1e-3
        above.  ``noise`` (K+1, B, Ta, Da) replaces the in-kernel draws.  Returns (B, Ta, Da)."""
        if "rgb" in cond:
            raise NotImplementedError("dppo_amd: QSM is built for state observations only (like the reference)")
        return self._run_sampler(cond, bool(deterministic), False, False, noise, None, "QSMDiffusion.forward").trajectories
