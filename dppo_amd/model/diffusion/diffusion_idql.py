"""Implicit diffusion Q-learning.  Mirrors ``dppo/model/diffusion/diffusion_idql.py`` (reference ``IDQLDiffusion``) on top of
``RWRDiffusion``'s sampling schedule (``diffusion_rwr.py:65-103``: std clipped at ``min_sampling_denoising_std``, which is
``DiffusionModel._sampling_schedule`` with no fine-tuned steps).

The actor's loss is the inherited denoising MSE.  The critics' losses, the Polyak target and the best-of-N action selection
are library calls (csrc/idql.hip): ``loss_critic_v`` / ``loss_critic_q`` leave the flat gradient in the critic's
``flat_grads()`` and return the loss through the same autograd shim as ``DiffusionModel.loss``; ``forward`` queues the sampler,
the target twin, V and the selection without a host synchronisation in between."""
from __future__ import annotations

import copy
import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.diffusion.diffusion import DiffusionModel
from dppo_amd.util.replay import DeviceReplay


class IDQLDiffusion(DiffusionModel):
    def __init__(self, actor, critic_q, critic_v, min_sampling_denoising_std=0.1, use_ddim=False, **kwargs):
        super().__init__(network=actor, use_ddim=use_ddim, **kwargs)
        assert not self.use_ddim, "RWR does not support DDIM"  # (the reference's message: diffusion_rwr.py:27)
        self.min_sampling_denoising_std = min_sampling_denoising_std
        self.critic_q = critic_q.to(self.device)
        self.target_q = copy.deepcopy(critic_q).to(self.device)
        self.critic_v = critic_v.to(self.device)
        self.actor = self.network
        if self.critic_q.cond_dim != self.critic_v.cond_dim:
            raise ValueError("critic_q and critic_v observe different cond_dim")
        object.__setattr__(self, "_ws_v", hip.Workspace())
        object.__setattr__(self, "_ws_q", hip.Workspace())

    # ------------------------------------------------------------------ RL training (reference :42-95)
    def _v_call(self, obs, actions, inds, expectile, want_adv):
        q, v, tq = self.critic_q, self.critic_v, self.target_q
        batch, N, keep = off_policy.as_batch("IDQL", obs, inds, actions)
        lib, dq, dv = hip.load(), q.net_desc(), v.net_desc()
        dev = v.flat_params().device
        ws = self._ws_v.get(lib.dppo_idql_v_loss_workspace_bytes(C.byref(dq), C.byref(dv), self.prec, N, int(q.double_q)), dev,
                            "dppo_idql_v_loss_workspace_bytes")
        k1, k2 = tq.packed(self.prec)
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        adv = torch.empty(N, dtype=torch.float32, device=dev) if want_adv else None
        hip.check(lib.dppo_idql_v_loss_fwd_bwd(
            C.byref(dq), C.byref(dv), self.prec, tq.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2),
            v.flat_params().data_ptr(), v.packed(self.prec, 0).data_ptr(), C.byref(batch), N, float(expectile), int(q.double_q),
            v.flat_grads().data_ptr(), hip.ptr(adv), stats.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()),
            "dppo_idql_v_loss_fwd_bwd")
        return stats, adv

    @torch.no_grad()
    def compute_advantages(self, obs, actions, inds=None):
        """min(target q1, q2) - V per row, forward only (``dppo_idql_q_forward`` on the target twin and V's inference forward):
        no gradient buffer is touched.  ``obs`` may be a ``DeviceReplay`` with ``inds``, like the losses."""
        if isinstance(obs, DeviceReplay):
            rows = torch.arange(len(obs), device=obs.obs.device) if inds is None else inds
            st, _, actions, _, _ = obs.gather(rows)
        else:
            st = off_policy.state_of(obs, "IDQL")
        st = st.reshape(st.shape[0], -1)
        qs = self.target_q(st, actions)
        q = torch.minimum(*qs) if self.target_q.double_q else qs
        return q - self.critic_v(st).reshape(-1)

    def loss_critic_v(self, obs, actions, inds=None, expectile=0.8, want_adv=False):
        """mean(where(adv > 0, expectile, 1 - expectile) * adv^2); d loss / d V parameters in ``critic_v.flat_grads()``.
        ``last_stats``: {loss, mean adv, share of adv > 0} (device doubles); ``want_adv``: the epilogue's per-row adv in
        ``last_adv``."""
        stats, adv = self._v_call(obs, actions, inds, expectile, want_adv)
        object.__setattr__(self, "last_adv", adv)
        return off_policy.critic_loss(self, self.critic_v, stats)

    def loss_critic_q(self, obs, next_obs, actions, rewards, terminated, gamma, inds=None):
        """mean((q1 - y)^2) + mean((q2 - y)^2), y = r + gamma V(s') (1 - terminated); d loss / d [Q1 | Q2] parameters in
        ``critic_q.flat_grads()``.  ``last_stats``: {loss, mean q1, mean y}."""
        q, v = self.critic_q, self.critic_v
        batch, N, keep = off_policy.as_batch("IDQL", obs, inds, actions, next_obs, rewards, terminated)
        lib, dq, dv = hip.load(), q.net_desc(), v.net_desc()
        dev = v.flat_params().device
        ws = self._ws_q.get(lib.dppo_idql_q_loss_workspace_bytes(C.byref(dq), C.byref(dv), self.prec, N, int(q.double_q)), dev,
                            "dppo_idql_q_loss_workspace_bytes")
        k1, k2 = q.packed(self.prec)
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        hip.check(lib.dppo_idql_q_loss_fwd_bwd(
            C.byref(dq), C.byref(dv), self.prec, q.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2),
            v.flat_params().data_ptr(), v.packed(self.prec, 0).data_ptr(), C.byref(batch), N, float(gamma), int(q.double_q),
            q.flat_grads().data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_idql_q_loss_fwd_bwd")
        return off_policy.critic_loss(self, q, stats)

    @torch.no_grad()
    def update_target_critic(self, tau):
        off_policy.polyak(self.target_q, self.critic_q, tau)

    # ------------------------------------------------------------------ sampling (reference :125-188)
    @torch.no_grad()
    def forward(self, cond, deterministic=False, num_sample=10, critic_hyperparam=0.7, use_expectile_exploration=True,
                noise=None, u=None, return_all=False):
        """Best of ``num_sample`` candidates per observation: argmax of the target twin's min(q1, q2) when ``deterministic`` or
        without expectile exploration, else an index drawn with weights (adv > 0 ? critic_hyperparam : 1 - critic_hyperparam).
        ``noise`` (K+1, S*B, Ta, Da) and ``u`` (B,) replace the in-kernel draws (parity runs); candidates are sample-major,
        row s * B + b.  Returns (B, Ta, Da); with ``return_all`` also (idx (B,) int32, candidates, q1, q2, v)."""
        if "rgb" in cond:
            raise NotImplementedError("dppo_amd: IDQL is built for state observations only (like the reference)")
        state = cond["state"]
        hip.require_gpu(state, "IDQLDiffusion.forward")
        B, S, dev = state.shape[0], int(num_sample), state.device
        AF = self.horizon_steps * self.action_dim
        obs = state.reshape(B, -1).contiguous().float()
        cand = self._run_sampler({"state": obs.repeat(S, 1)}, bool(deterministic), False, False, noise, None,
                                 "IDQLDiffusion.forward").trajectories
        qs = self.target_q(obs, cand, obs_repeat=S)
        q1, q2 = qs if self.target_q.double_q else (qs, None)
        mode = 0 if deterministic or not use_expectile_exploration else 1
        v = self.critic_v(obs).reshape(B) if mode == 1 else None
        actions = torch.empty(B, AF, dtype=torch.float32, device=dev)
        idx = torch.empty(B, dtype=torch.int32, device=dev)
        seed = 0
        if mode == 1 and u is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        elif u is not None:
            u = u.reshape(B).contiguous().float()
        hip.check(hip.load().dppo_idql_select(q1.data_ptr(), hip.ptr(q2), hip.ptr(v), 1, cand.data_ptr(), hip.ptr(u), B, S, AF,
                                              mode, float(critic_hyperparam), seed, actions.data_ptr(), idx.data_ptr(),
                                              hip.stream()), "dppo_idql_select")
        actions = actions.view(B, self.horizon_steps, self.action_dim)
        return (actions, idx, cand, q1, q2, v) if return_all else actions
