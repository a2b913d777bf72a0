"""Calibrated conservative Q-learning (Cal-QL) with SAC's tanh-Gaussian policy.  Mirrors ``dppo/model/rl/gaussian_calql.py`` (reference
``CalQL_Gaussian``): ``network``, ``critic`` and ``target_critic`` under the reference's names.

The critic of every shipped Cal-QL cfg is ``CriticObsAct(use_layernorm: True, double_q: True)``: a TWIN of LayerNorm trunks, which
``CriticObsAct`` builds under ``twin_layernorm=True``.  ``child_node_defaults`` below asks the cfg loader for it, so a shipped cfg
builds with its text unchanged.  ``loss_critic`` is one library call (``dppo_calql_q_loss_fwd_bwd``, csrc/calql.hip): the TD loss
against the max over ``cql_n_actions`` policy samples of the target twin's min, plus the conservative term -- a logsumexp over random
actions and two policy samples whose Q is floored by the Monte-Carlo return -- for each trunk.

A fact about the reference, imitated by default: it subtracts ``log_pi`` (N,) from a (N, 1) column, so each row's logsumexp runs over
the WHOLE batch's log-probabilities; its loss equals the per-row form with ``-log_pi[n]`` replaced by the scalar ``logsumexp_m(-log_pi
[m])`` (csrc/calql.h).  ``per_row_logpi=True`` gives the Cal-QL paper's per-row importance weights instead.

``loss_actor`` is one library call too (``dppo_calql_actor_fwd_bwd``): SAC's reparameterised sample, both trunks' forwards, a per-row
select of the smaller Q (a tie splits in halves, ``torch.minimum``'s backward) that seeds RLPD's action-gradient chains through
LayerNorm, one tail whose epilogue is SAC's head backward, then the actor's backward.  It runs on the GPU only; on a CPU model it
raises ``NotImplementedError``.  ``forward``, ``loss_temperature`` and ``update_target_critic`` are SAC's.  The agent is
``dppo_amd.agent.finetune.train_calql_agent.TrainCalQLAgent``."""
from __future__ import annotations

import copy
import ctypes as C
import logging

import numpy as np
import torch

from dppo_amd import hip
from dppo_amd.model.common import off_policy
from dppo_amd.model.rl.gaussian_sac import SAC_Gaussian
from dppo_amd.util.replay import DeviceReplay

log = logging.getLogger(__name__)


class CalQL_Gaussian(SAC_Gaussian):
    child_node_defaults = {"critic": {"twin_layernorm": True}}  # read by dppo_amd.cfg.loader.instantiate
    n_random_actions = 10  # ``loss_critic(random_actions=None)`` draws this many per row (the shipped cfgs' train.n_random_actions)

    def __init__(self, actor, critic, network_path=None, cql_clip_diff_min=-np.inf, cql_clip_diff_max=np.inf, cql_min_q_weight=5.0,
                 cql_n_actions=10, per_row_logpi=False, **kwargs):
        if not getattr(critic, "twin_layernorm", False):
            raise ValueError("Cal-QL's critic is the twin of LayerNorm trunks: CriticObsAct(use_layernorm=True, double_q=True, "
                             "twin_layernorm=True), as every shipped calql_mlp_*.yaml configures it")
        super().__init__(actor=actor, critic=critic, network_path=None, **kwargs)
        self.cql_clip_diff_min, self.cql_clip_diff_max = float(cql_clip_diff_min), float(cql_clip_diff_max)
        self.cql_min_q_weight, self.cql_n_actions = float(cql_min_q_weight), int(cql_n_actions)
        self.per_row_logpi = bool(per_row_logpi)
        if network_path is not None:  # actor, critic and target critic (reference :41-51)
            checkpoint = torch.load(network_path, map_location=self.device, weights_only=True)  # safe loader only
            self.load_state_dict(checkpoint["model"], strict=True)
            log.info("Loaded actor and critics from %s", network_path)
        object.__setattr__(self, "_ws_calql", hip.Workspace())

    def loss_critic(self, obs, next_obs, actions, random_actions, rewards, returns, terminated, gamma, inds=None, samples=None,
                    noise=None):
        """td_1 + td_2 + w mean(diff_1) + w mean(diff_2) (reference :56-171; csrc/calql.h states the arithmetic), d loss / d [Q1 | Q2]
        parameters in ``critic.flat_grads()``; ``last_stats``: {loss, td_1 + td_2, mean diff_1, mean diff_2, mean q1, mean y};
        ``last_y`` (N,).  ``obs`` may be a ``DeviceReplay`` (rows ``inds``); ``returns`` is a tensor (N,).  ``random_actions`` (N, R,
        Ta, Da), or None: ``n_random_actions`` per row are drawn in the kernel, uniform in [-1, 1), and left in
        ``last_random_actions``.  ``samples``: dict(next_actions (N S, Ta, Da), pi_actions (N, Ta, Da), log_pi (N,), pi_next_actions,
        log_pi_next); without it the three policy samples come from ONE ``forward`` over N (S + 2) stacked rows [next_obs each S
        times | obs | next_obs] (the reference's call order), ``noise`` (N (S + 2), Ta, Da) replacing its draws."""
        q, tq, S = self.critic, self.target_critic, self.cql_n_actions
        batch, N, keep = off_policy.as_batch("Cal-QL", obs, inds, actions, next_obs, rewards, terminated)
        dev = q.flat_params().device
        lib, dq = hip.load(), q.net_desc()
        OD = q.cond_dim
        AF = dq.in_dim - OD
        if samples is None:
            if isinstance(obs, DeviceReplay):
                cur, nxt = off_policy.rows_of("Cal-QL", obs, inds), off_policy.rows_of("Cal-QL", obs, inds, nxt=True)
            else:
                cur, nxt = off_policy.state_of(obs, "Cal-QL"), off_policy.state_of(next_obs, "Cal-QL")
            cur, nxt = cur.reshape(N, -1), nxt.reshape(N, -1)
            a, lp = self.forward({"state": torch.cat([nxt.repeat_interleave(S, dim=0), cur, nxt])}, deterministic=False,
                                 get_logprob=True, noise=noise)
            a = a.reshape(N * (S + 2), AF)
            samples = dict(next_actions=a[:N * S], pi_actions=a[N * S:N * S + N], log_pi=lp[N * S:N * S + N],
                           pi_next_actions=a[N * S + N:], log_pi_next=lp[N * S + N:])
        flat = lambda x, *s: x.reshape(*s).contiguous().float()
        next_a, pi_a, pi_na = flat(samples["next_actions"], N * S, AF), flat(samples["pi_actions"], N, AF), flat(samples["pi_next_actions"], N, AF)
        lp, lpn, returns = flat(samples["log_pi"], N), flat(samples["log_pi_next"], N), flat(returns, N)
        hip.require_gpu(returns, "CalQL_Gaussian.loss_critic")
        cfg = hip.CalqlCfg(n_next=S, per_row_logpi=int(self.per_row_logpi), min_q_weight=self.cql_min_q_weight,
                           clip_diff_min=self.cql_clip_diff_min, clip_diff_max=self.cql_clip_diff_max, log_rand_pi=0.5 ** AF)
        if random_actions is None:
            R = int(self.n_random_actions)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
            cfg.seed_lo, cfg.seed_hi = seed & 0xFFFFFFFF, seed >> 32
            random_out = torch.empty(N, R, self.horizon_steps, AF // self.horizon_steps, dtype=torch.float32, device=dev)
        else:
            R, random_out = random_actions.shape[1], None
            random_actions = flat(random_actions, N * R, AF)
        cfg.n_random = R
        ws = self._ws_calql.get(lib.dppo_calql_q_loss_workspace_bytes(C.byref(dq), self.prec, OD, N, R, S), dev,
                                "dppo_calql_q_loss_workspace_bytes")
        k1, k2 = q.packed(self.prec)
        t1, t2 = tq.packed(self.prec)
        stats = torch.empty(hip.CALQL_STAT_COUNT, dtype=torch.float64, device=dev)
        y = torch.empty(N, dtype=torch.float32, device=dev)
        hip.check(lib.dppo_calql_q_loss_fwd_bwd(
            C.byref(dq), self.prec, q.flat_params().data_ptr(), k1.data_ptr(), k2.data_ptr(), tq.flat_params().data_ptr(),
            t1.data_ptr(), t2.data_ptr(), C.byref(cfg), C.byref(batch), OD, returns.data_ptr(), next_a.data_ptr(), pi_a.data_ptr(),
            lp.data_ptr(), pi_na.data_ptr(), lpn.data_ptr(), hip.ptr(random_actions), N, float(gamma), q.flat_grads().data_ptr(),
            stats.data_ptr(), y.data_ptr(), hip.ptr(random_out), ws.data_ptr(), ws.numel(), hip.stream()),
            "dppo_calql_q_loss_fwd_bwd")
        object.__setattr__(self, "last_y", y)
        object.__setattr__(self, "last_random_actions", random_out)
        return off_policy.critic_loss(self, q, stats)

    def loss_actor(self, obs, alpha, inds=None, noise=None):
        """mean(-min(q1, q2)(s, a) + alpha logp(a)) on a reparameterised sample (reference :173-182), and d loss / d actor parameters
        in ``last_loss_grad``; nothing of the critic's is written.  ``noise`` (N, Ta, Da) replaces the draws.  ``last_stats``: {loss,
        mean q_sel, mean logp, mean sigma}; ``last_d_a`` (N, Ta*Da) = d loss / d a through the twin; ``last_logp`` (N,);
        ``last_actions`` (N, Ta*Da); ``last_sel`` (N,) bytes: 0 Q1 was taken, 1 Q2 (q2 < q1), 2 a tie (both at one half,
        ``torch.minimum``'s backward).  ``obs`` may be a ``DeviceReplay`` (rows ``inds``)."""
        if not next(self.network.parameters()).is_cuda:
            raise NotImplementedError("dppo_amd: Cal-QL's actor loss runs on the GPU only; a CPU path would be a follow-up and is "
                                      "not built")
        return self._loss_actor("Cal-QL", "dppo_calql_actor_workspace_bytes", "dppo_calql_actor_fwd_bwd", self.critic,
                                lambda: (self.critic.flat_params(), *self.critic.packed(self.prec)), (), True, obs, alpha, inds, noise)
