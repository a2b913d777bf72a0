"""Imitation-bootstrapped RL (IBRL) for a Gaussian policy.  Mirrors ``dppo/model/rl/gaussian_ibrl.py`` (reference
``IBRL_Gaussian``): ``network``, ``target_actor``, ``bc_policy``, ``critic_networks.{e}`` and ``target_networks.{e}`` under the
reference's names.

The actor is ``Gaussian_MLP(fixed_std=0.1)`` on a plain trunk with ``nn.Dropout`` behind every hidden Linear (seven of the eight
shipped cfgs: ``dropout: 0.5``), built under ``plain_fixed_std=True``, which ``child_node_defaults`` below asks the cfg loader for so
that a shipped cfg builds with its text unchanged.  The reference keeps the model in ``train()`` while it acts and trains, so dropout
is live in all three actors; here it follows each module's own mode, as torch's does.  The critics are RLPD's: E LayerNorm plain
trunks in one flat [E][P] buffer (``_Ensemble``), the targets in a second one.

``forward`` is one library call (``dppo_ibrl_act``, csrc/ibrl.hip): the frozen imitation policy's proposal, the online actor's, both
scored by the smaller Q of a random pair of online members, and the choice per row.  ``loss_critic`` is one call too
(``dppo_ibrl_q_loss_fwd_bwd``) behind the two next-action samples: the TD target bootstraps from the better of the two proposals
under the smaller Q of a random pair of target members; the loss, the members' backwards and the gradient layout are RLPD's.

Deviations from the reference, documented and not imitated:
  * its optimiser steps the stacked copies in ``ensemble_params``, so ``critic_networks.*`` in its checkpoints keep their INITIAL
    values; here ``critic_networks.*`` are the trained parameters;
  * its state dict also carries ``base_model.*`` on the meta device; ``load_state_dict`` here accepts and ignores those keys;
  * in the soft choice, where both ``exp(beta q)`` overflow, ``w_rl - w_bc`` is NaN and the reference's ``torch.multinomial`` raises;
    here the greedy rule (BC iff ``q_bc > q_rl``) decides that row;
  * the soft choice draws one uniform ``u`` per row and takes BC iff ``u < p_bc`` with ``p_bc = 1 / (1 + exp(w_rl - w_bc))`` in
    fp32, where the reference hands the softmax of the two weights to ``torch.multinomial``: the same distribution, other draws.

``loss_actor`` is one call as well (``dppo_ibrl_actor_fwd_bwd``): the online actor's forward with dropout, the fixed-std head with its
tanh mean, all E members' forwards, the min per row (a tie goes to the lowest member index), every member's action-gradient chain
from a seed that is zero on the rows it did not win, one tail over E * hidden, the head's backward and the actor's backward through
its dropout masks.  It runs on the GPU only.  ``TrainIBRLAgent`` (agent/finetune/train_ibrl_agent.py) drives the three.

Not built: the dropout BC pre-training (``pre_gaussian_mlp_ibrl``; ``GaussianModel.loss`` refuses the plain fixed-std actor), pixel
observations."""
from __future__ import annotations

import copy
import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.common.ensemble import EnsembleCritics
from dppo_amd.model.common.gaussian import GaussianModel
from dppo_amd.model.diffusion.diffusion import _FusedDenoiseLoss, flat_views


class IBRL_Gaussian(EnsembleCritics, GaussianModel):
    child_node_defaults = {"actor": {"plain_fixed_std": True}}  # read by dppo_amd.cfg.loader.instantiate

    def __init__(self, actor, critic, n_critics, soft_action_sample=False, soft_action_sample_beta=10, **kwargs):
        if not getattr(actor, "plain_fixed_std", False):
            raise ValueError("IBRL's actor is the plain fixed-std trunk: Gaussian_MLP(fixed_std=..., residual_style=False, "
                             "plain_fixed_std=True), as every shipped ibrl_mlp*.yaml configures it")
        if getattr(critic, "double_q", True):
            raise ValueError("IBRL's members are single critics (double_q=False): the reference's loss reads one output of each")
        if not 2 <= n_critics <= hip.RLPD_MAX_E:
            raise ValueError(f"IBRL needs n_critics in [2, {hip.RLPD_MAX_E}]: the Q of a proposal is the smaller of a random pair")
        dq = critic.net_desc()
        if not (dq.plain and dq.use_layernorm):
            raise ValueError("IBRL's members are LayerNorm plain trunks: CriticObsAct(use_layernorm=True, double_q=False)")
        super().__init__(network=actor, **kwargs)  # loads network_path into ``network`` first: the copies below start from it
        self.soft_action_sample, self.soft_action_sample_beta = bool(soft_action_sample), float(soft_action_sample_beta)
        self.target_actor = copy.deepcopy(self.network)
        self.bc_policy = copy.deepcopy(self.network)
        for p in self.bc_policy.parameters():
            p.requires_grad = False
        self._init_ensemble(critic, n_critics)
        for name in ("_ws_act", "_ws_q", "_ws_actor"):
            object.__setattr__(self, name, hip.Workspace())

    def update_target_actor(self, tau):
        """target_actor <- target_actor * (1 - tau) + network * tau over the actor's flat image in one call."""
        off_policy.polyak(self.target_actor, self.network, tau)

    @staticmethod
    def _seed():
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        return seed & 0xFFFFFFFF, seed >> 32

    # ------------------------------------------------------------------ acting (reference :149-205)
    @torch.no_grad()
    def forward(self, cond, deterministic=False, reparameterize=False, *, pair=None, noise_bc=None, noise_rl=None, mask_bc=None,
                mask_rl=None, u=None):
        """cond {"state": (B, To, Do)} -> the action chunk (B, Ta, Da): per row the frozen imitation policy's proposal (sigma 1e-4)
        or the online actor's, whichever the smaller Q of the online members ``pair`` (or ``get_random_indices()``) prefers --
        greedily when ``deterministic`` or not ``soft_action_sample`` (BC iff q_bc > q_rl: a tie or a NaN takes RL), otherwise by a
        two-way draw with weights exp(beta q).  ``reparameterize`` changes nothing without a gradient and is accepted as the
        reference's callers pass it.  ``noise_*`` (B, Ta, Da), ``mask_*`` (L, B, H) uint8 and ``u`` (B,) replace the draws.  Leaves
        ``last_q_bc``, ``last_q_rl`` (B,), ``last_took_bc`` (B,) bool, ``last_a_bc``, ``last_a_rl`` (B, Ta*Da), ``last_pair``."""
        state = off_policy.state_of(cond, "IBRL")
        hip.require_gpu(state, "IBRL_Gaussian.forward")
        if pair is None:
            pair = self.get_random_indices()
        p0, p1 = int(pair[0]), int(pair[1])
        net, bc, q = self.network, self.bc_policy, self.critic_networks[0]
        B, dev = state.shape[0], state.device
        AF = net.action_dim * net.horizon_steps
        obs = state.reshape(B, -1).contiguous().float()
        lib, da, dq = hip.load(), net.net_desc(), q.net_desc()
        cfg_bc = bc.gaussian_cfg(deterministic=True, randn_clip=self.randn_clip_value)
        cfg_rl = net.gaussian_cfg(deterministic=deterministic, randn_clip=self.randn_clip_value)
        if noise_bc is None:
            cfg_bc.seed_lo, cfg_bc.seed_hi = self._seed()
        else:
            noise_bc = noise_bc.reshape(B, AF).contiguous().float()
        if noise_rl is None:
            cfg_rl.seed_lo, cfg_rl.seed_hi = self._seed()
        else:
            noise_rl = noise_rl.reshape(B, AF).contiguous().float()
        drop_bc, keep_b, _ = self._dropout_of(bc, B, dev, mask_bc)
        drop_rl, keep_r, _ = self._dropout_of(net, B, dev, mask_rl)
        soft = self.soft_action_sample and not deterministic
        s_lo = s_hi = 0
        if u is not None:
            u = u.reshape(B).contiguous().float()
        elif soft:
            s_lo, s_hi = self._seed()
        ws = self._ws_act.get(lib.dppo_ibrl_act_workspace_bytes(C.byref(da), C.byref(dq), self.prec, B), dev,
                              "dppo_ibrl_act_workspace_bytes")
        qk, keep_q = self._ens.images(self.prec)
        action, a_bc, a_rl = (torch.empty(B, AF, dtype=torch.float32, device=dev) for _ in range(3))
        q_bc, q_rl = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(2))
        took = torch.empty(B, dtype=torch.uint8, device=dev)
        hip.check(lib.dppo_ibrl_act(
            C.byref(da), C.byref(dq), self.prec, self.n_critics, bc.flat_params().data_ptr(), bc.packed(self.prec, 0).data_ptr(),
            net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(), C.byref(cfg_bc), C.byref(cfg_rl),
            C.byref(drop_bc) if drop_bc is not None else None, C.byref(drop_rl) if drop_rl is not None else None,
            self.critic_flat_params().data_ptr(), qk, p0, p1, obs.data_ptr(), hip.ptr(noise_bc), hip.ptr(noise_rl), B, int(soft),
            self.soft_action_sample_beta, hip.ptr(u), s_lo, s_hi, action.data_ptr(), a_bc.data_ptr(), a_rl.data_ptr(),
            q_bc.data_ptr(), q_rl.data_ptr(), took.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_ibrl_act")
        for name, v in (("last_q_bc", q_bc), ("last_q_rl", q_rl), ("last_took_bc", took.bool()), ("last_a_bc", a_bc),
                        ("last_a_rl", a_rl), ("last_pair", (p0, p1))):
            object.__setattr__(self, name, v)
        return action.view(B, self.horizon_steps, -1)

    # ------------------------------------------------------------------ RL training (reference :69-128)
    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, inds=None, *, pair=None, next_actions_bc=None,
                    next_actions_rl=None, noise_bc=None, noise_rl=None, mask_bc=None, mask_rl=None):
        """mean over E N of (q_e - y)^2, y = r + gamma (1 - terminated) tq, tq = the better of min(tq_i, tq_j)(s', a'_bc) and
        min(tq_i, tq_j)(s', a'_rl) (BC iff strictly greater), (i, j) = ``pair`` or ``get_random_indices()``, a'_bc ~ ``bc_policy``
        at sigma 1e-4 and a'_rl ~ ``target_actor``, both without gradient and with dropout per the module's mode.  d loss / d every
        member's parameters in ``critic_flat_grads()`` ([E][P]); ``last_stats``: {loss, mean q, mean y}; ``last_y`` (N,);
        ``last_bc_share`` (device double: the share of rows where BC won); ``last_pair``.  ``obs`` may be a ``DeviceReplay`` (rows
        ``inds``).  ``next_actions_*`` (N, Ta, Da) replace the samples, ``noise_*`` (N, Ta, Da) and ``mask_*`` (L, N, H) their draws."""
        (p0, p1), batch, N, keep = self._td_head("IBRL", pair, obs, inds, actions, next_obs, rewards, terminated)
        q = self.critic_networks[0]
        dev = self.critic_flat_params().device
        if next_actions_bc is None or next_actions_rl is None:
            nxt = self._next_cond("IBRL", obs, inds, next_obs, N)
            if next_actions_bc is None:
                next_actions_bc = self._sample(self.bc_policy, nxt, True, noise_bc, drop_mask=mask_bc)[0]
            if next_actions_rl is None:
                next_actions_rl = self._sample(self.target_actor, nxt, False, noise_rl, drop_mask=mask_rl)[0]
        next_actions_bc = next_actions_bc.reshape(N, -1).contiguous().float()
        next_actions_rl = next_actions_rl.reshape(N, -1).contiguous().float()
        lib, dq, E = hip.load(), q.net_desc(), self.n_critics
        OD = q.cond_dim
        assert next_actions_bc.shape[1] == next_actions_rl.shape[1] == dq.in_dim - OD, "next actions must be (N, Ta, Da)"
        ws = self._ws_q.get(lib.dppo_ibrl_q_loss_workspace_bytes(C.byref(dq), self.prec, OD, N, E), dev, "dppo_ibrl_q_loss_workspace_bytes")
        qk, keep_q = self._ens.images(self.prec)
        tk, keep_t = self._tens.images(self.prec)
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        y = torch.empty(N, dtype=torch.float32, device=dev)
        share = torch.empty((), dtype=torch.float64, device=dev)
        grads = self.critic_flat_grads()
        hip.check(lib.dppo_ibrl_q_loss_fwd_bwd(
            C.byref(dq), self.prec, E, self.critic_flat_params().data_ptr(), qk, self.target_flat_params().data_ptr(), tk, p0, p1,
            C.byref(batch), OD, next_actions_bc.data_ptr(), next_actions_rl.data_ptr(), N, float(gamma), grads.data_ptr(),
            stats.data_ptr(), y.data_ptr(), share.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_ibrl_q_loss_fwd_bwd")
        return self._td_tail(stats, grads, (p0, p1), last_y=y, last_bc_share=share)

    def loss_actor(self, obs, inds=None, *, noise=None, mask=None, want_mask=False):
        """-mean_n min_e q_e(s_n, a_n) on the online actor's reparameterised sample a = mu + fixed_std clamp(eps) (reference
        :115-128), and d loss / d actor parameters in ``last_loss_grad``: through the selected member alone, the tanh mean and the
        actor's dropout (live iff ``network.training`` and its ``dropout`` > 0).  The min is torch.min's: a tie goes to the lowest
        member index.  No member's gradient is touched.  ``noise`` (N, Ta, Da) and ``mask`` (L, N, H) uint8 replace the draws.
        ``last_stats``: {loss, mean of the min q, mean over rows and members of q}; ``last_d_a`` (N, Ta*Da) = d loss / d a;
        ``last_actions`` (N, Ta*Da); ``last_qmin`` (N,); ``last_sel`` (N,) bytes: the selected member; ``last_drop_mask`` (L, N, H)
        the mask used where ``want_mask`` asks for it and dropout is live, else None (the backward reads the workspace's copy).
        ``obs`` may be a ``DeviceReplay`` (rows ``inds``)."""
        net, q = self.network, self.critic_networks[0]
        if not next(net.parameters()).is_cuda:
            raise NotImplementedError("dppo_amd: IBRL's actor loss runs on the GPU only; a CPU path would be a follow-up and is "
                                      "not built")
        batch, N, keep = off_policy.as_batch("IBRL", obs, inds)
        dev = net.flat_params().device
        AF = self.horizon_steps * net.action_dim
        cfg = net.gaussian_cfg(deterministic=False, randn_clip=self.randn_clip_value)
        if noise is None:
            cfg.seed_lo, cfg.seed_hi = self._seed()
        else:
            noise = noise.reshape(N, AF).contiguous().float()
        drop, keep_m, mask_out = self._dropout_of(net, N, dev, mask, want_mask=want_mask)
        lib, da, dq, E = hip.load(), net.net_desc(), q.net_desc(), self.n_critics
        OD = q.cond_dim
        ws = self._ws_actor.get(lib.dppo_ibrl_actor_workspace_bytes(C.byref(da), C.byref(dq), self.prec, OD, N, E), dev,
                                "dppo_ibrl_actor_workspace_bytes")
        qk, keep_q = self._ens.images(self.prec)
        grad = torch.empty_like(net.flat_params())
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        d_a, actions = (torch.empty(N, AF, dtype=torch.float32, device=dev) for _ in range(2))
        qmin = torch.empty(N, dtype=torch.float32, device=dev)
        sel = torch.empty(N, dtype=torch.uint8, device=dev)
        hip.check(lib.dppo_ibrl_actor_fwd_bwd(
            C.byref(da), C.byref(dq), self.prec, E, net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(),
            self.critic_flat_params().data_ptr(), qk, C.byref(cfg), C.byref(drop) if drop is not None else None, C.byref(batch), OD, N,
            hip.ptr(noise), grad.data_ptr(), stats.data_ptr(), d_a.data_ptr(), actions.data_ptr(), qmin.data_ptr(), sel.data_ptr(),
            ws.data_ptr(), ws.numel(), hip.stream()), "dppo_ibrl_actor_fwd_bwd")
        for name, v in (("last_loss_grad", grad), ("last_stats", stats), ("last_d_a", d_a), ("last_actions", actions),
                        ("last_qmin", qmin), ("last_sel", sel), ("last_drop_mask", mask_out)):
            object.__setattr__(self, name, v)
        params = net.trunk_parameters()
        return _FusedDenoiseLoss.apply(stats[0], flat_views(grad, params), *params)
