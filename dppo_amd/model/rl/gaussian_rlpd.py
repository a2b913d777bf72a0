"""Reinforcement learning with prior data (RLPD): SAC's tanh-Gaussian actor against an ENSEMBLE of LayerNorm critics.  Mirrors
``dppo/model/rl/gaussian_rlpd.py`` (reference ``RLPD_Gaussian``): ``network``, ``critic_networks.{e}`` and ``target_networks.{e}``
under the reference's names.

The members are ``CriticObsAct(use_layernorm=True, double_q=False)`` deep copies.  All members' parameters are views of ONE flat
fp32 buffer [E][P] (the targets' of a second one), so one optimiser step over ``critic_flat_params()`` and one Polyak call serve
the ensemble.  ``loss_critic`` is one library call (``dppo_rlpd_q_loss_fwd_bwd``, csrc/rlpd.hip): the TD target from the pair of
target members the caller's CPU generator draws (``get_random_indices``: ``torch.randperm(E)[:2]``, as the reference), all E members'
forwards and parameter backwards.  ``forward``, ``loss_temperature`` and the sampling are SAC's.

Two facts about the reference, documented and not imitated:
  * its optimiser steps the stacked copies in ``ensemble_params``, so ``critic_networks.*`` in its checkpoints keep their INITIAL
    values; here ``critic_networks.*`` are the trained parameters;
  * its state dict also carries ``base_model.*`` on the meta device; ``load_state_dict`` here accepts and ignores those keys.

``loss_actor`` is one library call too (``dppo_rlpd_actor_fwd_bwd``): SAC's reparameterised sample, every member's forward and its
action-gradient chain through LayerNorm, one tail over E * hidden whose epilogue is SAC's head backward with the members' mean
dq/da, then the actor's backward.  It runs on the GPU only; on a CPU model it raises ``NotImplementedError``."""
from __future__ import annotations

import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.common.ensemble import EnsembleCritics, _Ensemble  # noqa: F401  (_Ensemble: imported from here too)
from dppo_amd.model.rl.gaussian_sac import SAC_Gaussian


class RLPD_Gaussian(EnsembleCritics, SAC_Gaussian):
    def __init__(self, actor, critic, n_critics, backup_entropy=False, **kwargs):
        if getattr(critic, "double_q", True):
            raise ValueError("RLPD's members are single critics (double_q=False): the reference's loss reads one output of each")
        if n_critics < 2:
            raise ValueError("RLPD needs at least two critics: the TD target is the smaller of a random pair")
        SAC_Gaussian._check_actor(actor)
        super(SAC_Gaussian, self).__init__(network=actor, **kwargs)  # GaussianModel's: SAC_Gaussian's own wants the twin critic
        self.backup_entropy = bool(backup_entropy)
        self._init_ensemble(critic, n_critics)
        for name in ("_ws_s", "_ws_actor", "_ws_q"):
            object.__setattr__(self, name, hip.Workspace())

    # ------------------------------------------------------------------ RL training (reference gaussian_rlpd.py:64-133)
    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, alpha, inds=None, next_actions=None, next_logp=None,
                    noise=None, pair=None):
        """mean over E N of (q_e - y)^2, y = r + gamma (1 - terminated) min(tq_i, tq_j)(s', a') [+ gamma (1 - terminated) alpha
        (-logp(a')) with ``backup_entropy``], (i, j) = ``pair`` or ``get_random_indices()``, a' ~ forward(s') without gradient.
        d loss / d every member's parameters in ``critic_flat_grads()`` ([E][P]); ``last_stats``: {loss, mean q, mean y}.  ``obs``
        may be a ``DeviceReplay`` (rows ``inds``).  ``next_actions`` (N, Ta, Da) with ``next_logp`` (N,), or ``noise`` (N, Ta, Da),
        replace the sample / its draws."""
        (p0, p1), batch, N, keep = self._td_head("RLPD", pair, obs, inds, actions, next_obs, rewards, terminated)
        q = self.critic_networks[0]
        dev = self.critic_flat_params().device
        if next_actions is None:
            next_actions, next_logp = self.forward(self._next_cond("RLPD", obs, inds, next_obs, N), deterministic=False,
                                                   get_logprob=True, noise=noise)
        next_actions = next_actions.reshape(N, -1).contiguous().float()
        if self.backup_entropy:
            assert next_logp is not None, "next_actions needs next_logp"
            next_logp, alpha = next_logp.reshape(N).contiguous().float(), self._dev_scalar(alpha, dev)
        else:
            next_logp = alpha = None
        lib, dq, E = hip.load(), q.net_desc(), self.n_critics
        OD = q.cond_dim
        assert next_actions.shape[1] == dq.in_dim - OD, "next_actions must be (N, Ta, Da)"
        ws = self._ws_q.get(lib.dppo_rlpd_q_loss_workspace_bytes(C.byref(dq), self.prec, OD, N, E), dev, "dppo_rlpd_q_loss_workspace_bytes")
        qk, keep_q = self._ens.images(self.prec)
        tk, keep_t = self._tens.images(self.prec)
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        grads = self.critic_flat_grads()
        hip.check(lib.dppo_rlpd_q_loss_fwd_bwd(
            C.byref(dq), self.prec, E, self.critic_flat_params().data_ptr(), qk, self.target_flat_params().data_ptr(), tk, p0, p1,
            C.byref(batch), OD, next_actions.data_ptr(), hip.ptr(next_logp), hip.ptr(alpha), N, float(gamma), grads.data_ptr(),
            stats.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_rlpd_q_loss_fwd_bwd")
        return self._td_tail(stats, grads, (p0, p1))

    def loss_actor(self, obs, alpha, inds=None, noise=None):
        """mean(-(1/E) sum_e q_e(s, a) + alpha logp(a)) on a reparameterised sample (reference :100-112), and d loss / d actor
        parameters in ``last_loss_grad``; no member's gradient is touched.  ``noise`` (N, Ta, Da) replaces the draws.
        ``last_stats``: {loss, mean of the members' mean q, mean logp, mean sigma}; ``last_d_a`` (N, Ta*Da) = d loss / d a through
        the ensemble; ``last_logp`` (N,); ``last_actions`` (N, Ta*Da).  ``obs`` may be a ``DeviceReplay`` (rows ``inds``)."""
        if not next(self.network.parameters()).is_cuda:
            raise NotImplementedError("dppo_amd: RLPD's actor loss runs on the GPU only; a CPU path is not built")
        return self._loss_actor("RLPD", "dppo_rlpd_actor_workspace_bytes", "dppo_rlpd_actor_fwd_bwd", self.critic_networks[0],
                                lambda: (self.critic_flat_params(), self._ens.images(self.prec)[0]), (self.n_critics,), False, obs,
                                alpha, inds, noise)
