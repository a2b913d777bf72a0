"""Soft actor-critic with a tanh-Gaussian policy.  Mirrors ``dppo/model/rl/gaussian_sac.py`` (reference ``SAC_Gaussian``): same
attribute names (``network``, ``critic``, ``target_critic``), so the state dict is the reference's 34 keys.

The actor is a ``Gaussian_MLP`` with the state-dependent std (``fixed_std=None``, ``tanh_output=False``): the sample is squashed
AFTER the draw and its log-probability is a SUM over Ta*Da (``GaussianModel.forward``, reference gaussian.py:85-120).  Every loss
is one library call (csrc/sac.hip): ``loss_critic`` the TD loss with the entropy term in its bootstrap, ``loss_actor`` the
reparameterised ``mean(-min(Q1, Q2) + alpha logp)`` whose gradient reaches the actor through the critic's ACTION input (no
parameter gradient of the critic is computed), ``loss_temperature`` ``-mean(alpha (logp + target_entropy))``.  ``alpha`` and
``log_alpha`` are device float64 scalars: where the reference calls ``.item()`` once per update, nothing here reads the device.
The actor's flat gradient is left in ``last_loss_grad`` like ``GaussianModel.loss``, the critic's in ``critic.flat_grads()``."""
from __future__ import annotations

import copy
import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.common.gaussian import GaussianModel
from dppo_amd.model.diffusion.diffusion import _FusedDenoiseLoss, flat_views
from dppo_amd.util.replay import DeviceReplay


class SAC_Gaussian(GaussianModel):
    _squash_built = True

    @staticmethod
    def _check_actor(actor):
        if getattr(actor, "is_vision", False):
            raise NotImplementedError("dppo_amd: SAC is built for state observations only (like the reference)")
        if getattr(actor, "use_fixed_std", True):
            raise NotImplementedError("dppo_amd: SAC needs the state-dependent std (Gaussian_MLP with fixed_std=None, "
                                      "tanh_output=False): every shipped SAC / RLPD / Cal-QL / IBRL cfg has it")

    def __init__(self, actor, critic, **kwargs):
        self._check_actor(actor)
        if not getattr(critic, "double_q", False):
            raise ValueError("SAC needs the twin critic (double_q=True): the reference's SAC_Gaussian unpacks two outputs")
        super().__init__(network=actor, **kwargs)
        self.critic = critic.to(self.device)
        self.target_critic = copy.deepcopy(self.critic).to(self.device)
        for name in ("_ws_s", "_ws_actor", "_ws_q"):
            object.__setattr__(self, name, hip.Workspace())

    @staticmethod
    def _dev_scalar(x, dev):
        """alpha / log_alpha as a device float64 tensor (a Python number is uploaded, never read back)."""
        if torch.is_tensor(x):
            return x.detach().to(device=dev, dtype=torch.float64).reshape(-1)[:1].contiguous()
        return torch.full((1,), float(x), dtype=torch.float64, device=dev)

    def _cfg(self, deterministic, noise):
        cfg = self.network.sac_cfg(deterministic=deterministic, randn_clip=self.randn_clip_value, squash=self.tanh_output)
        if noise is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
            cfg.seed_lo, cfg.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        return cfg

    # ------------------------------------------------------------------ sampling (reference gaussian.py:85-120)
    @torch.no_grad()
    def forward(self, cond, deterministic=False, network_override=None, reparameterize=False, get_logprob=False, noise=None,
                want_u=False):
        """cond {"state": (B, To, Do)} -> the squashed sample (B, Ta, Da), with ``get_logprob`` (sample, logp (B,)).
        ``reparameterize`` changes nothing about the VALUE (the gradient through the sample is ``loss_actor``'s business).
        ``noise`` (B, Ta, Da) replaces the in-kernel draws; ``want_u``: the pre-squash sample in ``last_u``."""
        net = network_override if network_override is not None else self.network
        state = off_policy.state_of(cond, "SAC")
        hip.require_gpu(state, type(self).__name__ + ".forward")
        B, dev = state.shape[0], state.device
        AF = net.action_dim * net.horizon_steps
        obs = state.reshape(B, -1).contiguous().float()
        lib, d = hip.load(), net.net_desc()
        cfg = self._cfg(deterministic, noise)
        if noise is not None:
            noise = noise.reshape(B, AF).contiguous().float()
        actions = torch.empty(B, AF, device=dev)
        logp = torch.empty(B, device=dev) if get_logprob else None
        u = torch.empty(B, AF, device=dev) if want_u else None
        ws = self._ws_s.get(lib.dppo_sac_sample_workspace_bytes(C.byref(d), self.prec, B), dev, "dppo_sac_sample_workspace_bytes")
        hip.check(lib.dppo_sac_sample(
            C.byref(d), self.prec, net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(), C.byref(cfg), obs.data_ptr(),
            hip.ptr(noise), B, actions.data_ptr(), hip.ptr(logp), hip.ptr(u), ws.data_ptr(), ws.numel(), hip.stream()),
            "dppo_sac_sample")
        object.__setattr__(self, "last_u", u)
        actions = actions.view(B, self.horizon_steps, -1)
        return (actions, logp) if get_logprob else actions

    # ------------------------------------------------------------------ RL training (reference gaussian_sac.py:31-88)
    def loss_critic(self, obs, next_obs, actions, rewards, terminated, gamma, alpha, inds=None, next_actions=None, next_logp=None,
                    noise=None):
        """mean((q1 - y)^2) + mean((q2 - y)^2), y = r + gamma (min(target q1, q2)(s', a') - alpha logp(a')) (1 - terminated),
        a' ~ forward(s') without gradient; d loss / d [Q1 | Q2] parameters in ``critic.flat_grads()``, ``last_stats``: {loss,
        mean q1, mean y}.  ``obs`` may be a ``DeviceReplay`` (rows ``inds``).  ``next_actions`` (N, Ta, Da) with ``next_logp``
        (N,), or ``noise`` (N, Ta, Da), replace the sample / its draws."""
        q, tq = self.critic, self.target_critic
        batch, N, keep = off_policy.as_batch("SAC", obs, inds, actions, next_obs, rewards, terminated)
        dev = q.flat_params().device
        if next_actions is None:
            nxt = off_policy.rows_of("SAC", obs, inds, nxt=True) if isinstance(obs, DeviceReplay) else off_policy.state_of(next_obs, "SAC")
            next_actions, next_logp = self.forward({"state": nxt.reshape(N, -1)}, deterministic=False, get_logprob=True, noise=noise)
        assert next_logp is not None, "next_actions needs next_logp"
        next_actions = next_actions.reshape(N, -1).contiguous().float()
        next_logp = next_logp.reshape(N).contiguous().float()
        alpha = self._dev_scalar(alpha, dev)
        lib, dq = hip.load(), q.net_desc()
        OD = q.cond_dim
        assert next_actions.shape[1] == dq.in_dim - OD, "next_actions must be (N, Ta, Da)"
        ws = self._ws_q.get(lib.dppo_sac_q_loss_workspace_bytes(C.byref(dq), self.prec, OD, N), dev, "dppo_sac_q_loss_workspace_bytes")
        k1, k2 = q.packed(self.prec)
        t1, t2 = tq.packed(self.prec)
        stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
        hip.check(lib.dppo_sac_q_loss_fwd_bwd(
            C.byref(dq), self.prec, q.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2), tq.flat_params().data_ptr(),
            t1.data_ptr(), hip.ptr(t2), C.byref(batch), OD, next_actions.data_ptr(), next_logp.data_ptr(), alpha.data_ptr(), N,
            float(gamma), q.flat_grads().data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()),
            "dppo_sac_q_loss_fwd_bwd")
        return off_policy.critic_loss(self, q, stats)

    def loss_actor(self, obs, alpha, inds=None, noise=None):
        """mean(-min(q1, q2)(s, a) + alpha logp(a)) on a reparameterised sample, and d loss / d actor parameters in
        ``last_loss_grad``.  ``noise`` (N, Ta, Da) replaces the draws.  ``last_stats``: {loss, mean q_sel, mean logp, mean sigma};
        ``last_d_a`` (N, Ta*Da) = d loss / d a through the critic; ``last_logp`` (N,); ``last_sel`` (N,) bytes (1: Q2 was the
        smaller); ``last_actions`` (N, Ta*Da)."""
        return self._loss_actor("SAC", "dppo_sac_actor_workspace_bytes", "dppo_sac_actor_fwd_bwd", self.critic,
                                lambda: (self.critic.flat_params(), *self.critic.packed(self.prec)), (), True, obs, alpha, inds, noise)

    def _loss_actor(self, algo, ws_entry, entry, q, q_args, members, has_sel, obs, alpha, inds, noise):
        """What SAC's, Cal-QL's and RLPD's ``loss_actor`` share.  ``q``: the module whose descriptor the Q trunks have;
        ``q_args()``: the Q trunks' flat parameters, then the twin's two kernel images or the ensemble's image table with
        ``members`` = (E,); called behind the workspace query, where each of the three flattened and packed its critics."""
        net = self.network
        batch, N, keep = off_policy.as_batch(algo, obs, inds)
        dev = net.flat_params().device
        AF = self.horizon_steps * net.action_dim
        cfg = self._cfg(False, noise)
        if noise is not None:
            noise = noise.reshape(N, AF).contiguous().float()
        alpha = self._dev_scalar(alpha, dev)
        lib, da, dq = hip.load(), net.net_desc(), q.net_desc()
        OD = q.cond_dim
        ws = self._ws_actor.get(getattr(lib, ws_entry)(C.byref(da), C.byref(dq), self.prec, OD, N, *members), dev, ws_entry)
        q_params, *images = q_args()
        grad = torch.empty_like(net.flat_params())
        stats = torch.empty(hip.SAC_STAT_COUNT, dtype=torch.float64, device=dev)
        d_a = torch.empty(N, AF, dtype=torch.float32, device=dev)
        logp = torch.empty(N, dtype=torch.float32, device=dev)
        sel = torch.empty(N, dtype=torch.uint8, device=dev) if has_sel else None
        actions = torch.empty(N, AF, dtype=torch.float32, device=dev)
        hip.check(getattr(lib, entry)(
            C.byref(da), C.byref(dq), self.prec, *members, net.flat_params().data_ptr(), net.packed(self.prec, 0).data_ptr(),
            q_params.data_ptr(), *[hip.ptr(k) if torch.is_tensor(k) else k for k in images], C.byref(cfg), C.byref(batch), OD, N,
            hip.ptr(noise), alpha.data_ptr(), grad.data_ptr(), stats.data_ptr(), d_a.data_ptr(), logp.data_ptr(),
            *([sel.data_ptr()] if has_sel else []), actions.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), entry)
        for name, v in (("last_loss_grad", grad), ("last_stats", stats), ("last_d_a", d_a), ("last_logp", logp),
                        ("last_actions", actions)) + ((("last_sel", sel),) if has_sel else ()):
            object.__setattr__(self, name, v)
        params = net.trunk_parameters()
        return _FusedDenoiseLoss.apply(stats[0], flat_views(grad, params), *params)

    def loss_temperature(self, obs, log_alpha, target_entropy, inds=None, noise=None, logp=None):
        """-mean(alpha (logp + target_entropy)) with alpha = exp(log_alpha), logp of a fresh sample at ``obs`` without gradient
        (``logp`` (N,) given: that one).  ``log_alpha``: the device float64 leaf the reference exponentiates before the call;
        ``.backward()`` hands it d loss / d log_alpha, which also stays in ``last_alpha_out[1]``."""
        if logp is None:
            st = off_policy.rows_of("SAC", obs, inds)
            _, logp = self.forward({"state": st.reshape(st.shape[0], -1)}, deterministic=False, get_logprob=True, noise=noise)
        logp = logp.reshape(-1).contiguous().float()
        hip.require_gpu(logp, "SAC_Gaussian.loss_temperature")
        dev = logp.device
        assert torch.is_tensor(log_alpha) and log_alpha.dtype == torch.float64 and log_alpha.device == dev and log_alpha.numel() == 1
        out = torch.empty(2, dtype=torch.float64, device=dev)
        hip.check(hip.load().dppo_sac_alpha_loss(logp.data_ptr(), logp.numel(), log_alpha.data_ptr(), float(target_entropy),
                                                 out.data_ptr(), hip.stream()), "dppo_sac_alpha_loss")
        object.__setattr__(self, "last_alpha_out", out)
        return _FusedDenoiseLoss.apply(out[0], [out[1].reshape(log_alpha.shape)], log_alpha)

    def update_target_critic(self, tau):
        off_policy.polyak(self.target_critic, self.critic, tau)
