"""An ensemble of E critics in one flat [E][P] buffer, and the surface a model with such an ensemble and its targets offers
(RLPD_Gaussian, IBRL_Gaussian): the flat images one optimiser steps, the random pair, the Polyak step, the state dict."""
from __future__ import annotations

import copy
import ctypes as C

import torch
from torch import nn

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.diffusion.diffusion import _FusedDenoiseLoss, flat_views
from dppo_amd.util.replay import DeviceReplay


class _Ensemble:
    """E members of one architecture whose parameters are views of one flat [E][P] buffer, member e at [e P, (e + 1) P)."""

    def __init__(self, members):
        self.members = list(members)
        self._flat = self._grad = None

    def flat_params(self) -> torch.Tensor:
        ms = self.members
        own = [m.flat_params() for m in ms]
        P, flat = own[0].numel(), self._flat
        if flat is not None and all(o.data_ptr() == flat.data_ptr() + 4 * e * P for e, o in enumerate(own)):
            return flat
        flat = torch.empty(len(ms) * P, dtype=torch.float32, device=own[0].device)
        for e, m in enumerate(ms):  # re-home member e: its parameters, its flat image and its trunk's become slices of ``flat``
            sl = flat[e * P:(e + 1) * P]
            sl.copy_(own[e])
            off = 0
            for p in m.trunk_parameters():
                p.data = sl[off:off + p.numel()].view(p.shape)
                off += p.numel()
            object.__setattr__(m, "_flat", sl)
            m._packed.clear()
        self._flat = flat
        return flat

    def flat_grads(self) -> torch.Tensor:
        flat = self.flat_params()
        if self._grad is None or self._grad.device != flat.device or self._grad.numel() != flat.numel():
            self._grad = torch.zeros_like(flat)
        return self._grad

    def parameters(self):
        return [p for m in self.members for p in m.trunk_parameters()]

    def images(self, prec):
        """(ctypes array of the E kernel-image pointers, the tensors to keep alive)."""
        self.flat_params()
        bufs = [m.packed(prec)[0] for m in self.members]
        return (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs]), bufs

    def mark_updated(self):
        for m in self.members:
            m.mark_updated()


class EnsembleCritics:
    """Mixin of a model whose critics are E deep copies of one ``CriticObsAct(use_layernorm=True, double_q=False)`` with as many
    targets: ``critic_networks.{e}`` and ``target_networks.{e}`` under the reference's names, each set in one flat buffer."""

    def _init_ensemble(self, critic, n_critics):
        """Registers the two module lists (here in the constructor's order, which is the state dict's)."""
        self.n_critics = int(n_critics)
        self.critic_networks = nn.ModuleList([copy.deepcopy(critic).to(self.device) for _ in range(n_critics)])
        self.target_networks = nn.ModuleList([copy.deepcopy(critic).to(self.device) for _ in range(n_critics)])
        object.__setattr__(self, "_ens", _Ensemble(self.critic_networks))
        object.__setattr__(self, "_tens", _Ensemble(self.target_networks))

    def critic_flat_params(self) -> torch.Tensor:
        """[E][P] fp32: what one flat optimiser steps (call ``critics_updated()`` after a kernel wrote it behind torch's back)."""
        return self._ens.flat_params()

    def critic_flat_grads(self) -> torch.Tensor:
        return self._ens.flat_grads()

    def target_flat_params(self) -> torch.Tensor:
        return self._tens.flat_params()

    def critics_updated(self):
        self._ens.mark_updated()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """The reference's ``base_model.*`` (a stateless meta-device copy of one member) is accepted and ignored."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("base_model.")}, strict=strict, **kw)

    def get_random_indices(self, sz=None, num_ind=2):
        """``num_ind`` different members out of ``sz``, from torch's CPU generator (as the reference's); stays on the host: the
        pair is passed to the library by value."""
        return torch.randperm(self.n_critics if sz is None else sz)[:num_ind]

    def update_target_critic(self, tau):
        """target <- target * (1 - tau) + source * tau over the whole [E][P] image in one call."""
        t, s = self.target_flat_params(), self.critic_flat_params()
        hip.check(hip.load().dppo_polyak(t.data_ptr(), s.data_ptr(), float(tau), t.numel(), hip.stream()), "dppo_polyak")
        self._tens.mark_updated()

    # ------------------------------------------------------------------ the two ends of a loss_critic
    def _td_head(self, algo, pair, obs, inds, actions, next_obs, rewards, terminated):
        """-> the pair of target members (drawn if None) as two ints, the native batch, N, and what to keep alive."""
        if pair is None:
            pair = self.get_random_indices()
        batch, N, keep = off_policy.as_batch(algo, obs, inds, actions, next_obs, rewards, terminated)
        return (int(pair[0]), int(pair[1])), batch, N, keep

    @staticmethod
    def _next_cond(algo, obs, inds, next_obs, N):
        """The next observations' rows as a sampler's ``cond`` (for a caller that was not handed its next actions)."""
        nxt = off_policy.rows_of(algo, obs, inds, nxt=True) if isinstance(obs, DeviceReplay) else off_policy.state_of(next_obs, algo)
        return {"state": nxt.reshape(N, -1)}

    def _td_tail(self, stats, grads, pair, **last):
        """Leaves ``last_stats``, the caller's other ``last_*`` and ``last_pair``; -> the loss, whose backward hands out ``grads``."""
        for name, v in dict(last_stats=stats, **last, last_pair=pair).items():
            object.__setattr__(self, name, v)
        params = self._ens.parameters()
        return _FusedDenoiseLoss.apply(stats[0], flat_views(grads, params), *params)
