"""DPPO fine-tuning agent (entry point named by the north star).

Mirrors the reference's ``TrainPPODiffusionAgent`` / ``TrainPPOAgent`` / ``TrainAgent``
(agent/finetune/train_ppo_diffusion_agent.py:21-483, train_ppo_agent.py:16-89, train_agent.py:19-145): same cfg
keys, same iteration structure (rollout -> value / log-prob precompute -> reward scaling -> GAE -> epochs of
minibatch PPO with KL early stop -> LR schedules -> checkpoint), same checkpoint format.  What changed is WHERE
things live: the rollout buffer is fp32 and device-resident (the reference keeps float64 numpy holders and copies
them back and forth, :78-93,198-303), sampling / log-probs / GAE / gather + loss + backward / AdamW are HIP kernels,
and with WORLD_SIZE > 1 every rank owns a shard of the envs and gradients are all-reduced once per step
(dppo_amd.parallel).  Envs stay on host CPU.

This class is also what the four PPO agents share: ``run()``, the iteration, and ``_update()``, the update's skeleton (precompute,
reward scaling, GAE; epochs of minibatches with the KL early stop; the metrics).  What differs between them lies on two axes, each
a handful of small methods whose defaults here are this agent's, state observations and a denoising chain:

* observations (pixels: train_ppo_diffusion_img_agent.py): ``_collect``, ``_augment``, ``_cond``, ``_gather`` / ``_rows``,
  ``critic_kwargs``, ``_apply_gradients``, ``kl_stop_needs_actor``;
* sample (one-shot: ``OneShotSample`` in train_ppo_gaussian_agent.py): ``_policy``, ``_old_logprobs``, ``_minibatch``,
  ``_accumulate_logvar`` / ``_logvar_grad`` / ``_step_logvar``, ``_sample_metrics``.
"""
from __future__ import annotations

import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from dppo_amd import hip
from dppo_amd.agent.finetune.train_agent import TrainAgent
from dppo_amd.parallel import DataParallel
from dppo_amd.util.optim import FlatAdamW, step_and_repack
from dppo_amd.util.reward_scaling import RunningRewardScaler
from dppo_amd.util.rollout import collect_rollout, gae_device


class TrainPPODiffusionAgent(TrainAgent):
    log_line = "loss %8.4f | pg loss %8.4f | value loss %8.4f | reward %8.4f | t:%8.4f"
    log_keys = ("loss", "pg_loss", "v_loss", "train_episode_reward", "time")
    kl_stop_needs_actor = False  # whether the KL early stop waits for the critic warm-up to end (the pixel agents': yes)
    critic_kwargs = {}  # what the precompute's critic calls get beside the cond
    _bufs = None  # (observation buffer, chain buffer) of the rollout: device-resident, allocated by the first _collect

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv)
        # ---- TrainPPOAgent (train_ppo_agent.py:18-89)
        self.logprob_batch_size = cfg.train.get("logprob_batch_size", 10000)
        assert self.logprob_batch_size % self.n_envs == 0, "logprob_batch_size must be divisible by n_envs"
        self.n_critic_warmup_itr = cfg.train.n_critic_warmup_itr
        self.dp = DataParallel(self.model, self.world)
        if self.world > 1:
            # the broadcast above made the weights identical; from here on every rank needs its OWN random stream
            # (sampler Philox key, minibatch permutation, BC noise): same seed everywhere would give env row i of
            # every shard the same exploration noise
            self.reseed(self.seed + self.rank)
        self.actor_optimizer = FlatAdamW(self.model.actor_ft.flat_params(), lr=cfg.train.actor_lr,
                                         weight_decay=cfg.train.actor_weight_decay)
        self.critic_optimizer = FlatAdamW(self.model.critic.flat_params(), lr=cfg.train.critic_lr,
                                          weight_decay=cfg.train.critic_weight_decay)
        self.actor_lr_scheduler = self._cosine(self.actor_optimizer, cfg.train.actor_lr_scheduler, cfg.train.actor_lr)
        self.critic_lr_scheduler = self._cosine(self.critic_optimizer, cfg.train.critic_lr_scheduler, cfg.train.critic_lr)
        self.gae_lambda = cfg.train.get("gae_lambda", 0.95)
        self.target_kl = cfg.train.target_kl
        self.update_epochs = cfg.train.update_epochs
        self.ent_coef = cfg.train.get("ent_coef", 0)  # entropy of a fixed-variance chain is constant: no gradient
        self.vf_coef = cfg.train.get("vf_coef", 0)
        self.reward_scale_running = cfg.train.reward_scale_running
        if self.reward_scale_running:
            self.running_reward_scaler = RunningRewardScaler(self.n_envs, moments_hook=self._pool_return_moments)
        self.reward_scale_const = cfg.train.get("reward_scale_const", 1)
        self.use_bc_loss = cfg.train.get("use_bc_loss", False)
        self.bc_loss_coeff = cfg.train.get("bc_loss_coeff", 0)
        # ---- TrainPPODiffusionAgent (:22-45)
        self.reward_horizon = cfg.get("reward_horizon", self.act_steps)
        self.learn_eta = getattr(self.model, "learn_eta", False)

    @staticmethod
    def reseed(seed: int):
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)  # CPU generator (the sampler's Philox key is drawn from it) and the device generators

    # -------------------------------------------------------------------------------------------------
    def _pool_return_moments(self, mean, var, cnt):
        """Pool (mean, var, count) of the discounted returns over ranks (reward_scaling.py:52,65 pooled variance)."""
        if self.world == 1:
            return mean, var, cnt
        t = torch.tensor([cnt, cnt * mean, cnt * (var + mean * mean)], dtype=torch.float64, device=self.device)
        dist.all_reduce(t)
        n, s1, s2 = t.tolist()
        m = s1 / n
        return m, s2 / n - m * m, n

    def load(self, itr):
        data = torch.load(os.path.join(self.checkpoint_dir, f"state_{itr}.pt"), weights_only=True)
        self.itr = data["itr"]
        self.model.load_state_dict(data["model"])
        for net in (self.model.actor, self.model.actor_ft, self.model.critic):
            net.mark_updated()  # kernel images are rebuilt from the loaded weights on next use

    # ------------------------------------------------------------------------------------------------- the iteration
    def run(self):
        model = self.model
        S, E = self.n_steps, self.n_envs
        t_start = time.time()
        run_results = []
        cnt_train_step = 0
        last_itr_eval = False
        done_venv = np.zeros(E, dtype=bool)
        prev_obs = None
        metrics = {}
        while self.itr < self.n_train_itr:
            eval_mode = self.itr % self.val_freq == 0 and not self.force_train
            model.eval() if eval_mode else model.train()
            firsts = np.zeros((S + 1, E))
            if self.reset_at_iteration or eval_mode or last_itr_eval or prev_obs is None:
                prev_obs = self.reset_env_all()
                firsts[0] = 1
            else:
                firsts[0] = done_venv
            last_itr_eval = eval_mode
            # ---------------- rollout: sample on the GPU, step envs on the host (:101-151)
            reward_trajs, terminated_trajs, done_trajs, prev_obs = self._collect(prev_obs, eval_mode)
            firsts[1:] = done_trajs
            done_venv = done_trajs[-1].astype(bool)
            cnt_train_step += S * E * self.act_steps * self.world if not eval_mode else 0
            stats = self._episode_stats(firsts, reward_trajs)  # (:153-193)
            # ---------------- update (:196-390)
            if not eval_mode:
                metrics = self._update(*self._bufs, reward_trajs, terminated_trajs, firsts, prev_obs)
            # ---------------- schedules, annealing, checkpoint, logging (:406-483)
            if self.itr >= self.n_critic_warmup_itr:
                self.actor_lr_scheduler.step()
            self.critic_lr_scheduler.step()
            if hasattr(model, "step"):
                model.step()
            if self.itr % self.save_model_freq == 0 or self.itr == self.n_train_itr - 1:
                self.save_model()
            if self.itr % self.log_freq == 0 and self.rank == 0:
                self.log_record(run_results, {"itr": self.itr, "step": cnt_train_step}, t_start, eval_mode, stats, metrics)
            self.itr += 1
        return run_results

    def _chain_steps(self):
        """Kft.  0: a one-shot (Gaussian) policy, whose "chain" is the action itself."""
        return getattr(self.model, "ft_denoising_steps", 0)

    # ------------------------------------------------------------------------------------------------- observations: state
    def _collect(self, prev_obs, eval_mode):
        """One rollout of ``n_steps`` env steps into ``self._bufs``; -> (reward, terminated, done) as (S, E) numpy and the last
        observation.  Here: pinned hand-off, env groups (env.pipeline_groups) software-pipelined against the sampler
        (dppo_amd/util/rollout.py)."""
        if self._bufs is None:  # fp32, reused across iterations
            R = self.n_steps * self.n_envs
            self._bufs = (torch.empty(R, self.n_cond_step * self.obs_dim, device=self.device),
                          torch.empty(R, self._chain_steps() + 1, self.horizon_steps * self.action_dim, device=self.device))
        out = collect_rollout(self._policy(), self.venv, prev_obs, self.n_steps, self.act_steps, *self._bufs,
                              deterministic=eval_mode)
        if hasattr(self.model, "check_sampler_health"):
            self.model.check_sampler_health()  # fail loudly if the split sampler's hand-over ever timed out
        return out

    def _augment(self, obs_buf):
        """In front of everything that reads the buffer in an update."""

    def _cond(self, obs):
        """The env's observation dict (numpy) as the networks' cond."""
        return {"state": torch.from_numpy(obs["state"]).float().to(self.device)}

    def _gather(self, obs_buf, idx):
        """Rows ``idx`` (a slice or an index vector) of the observation buffer, as the one-shot ``ppo_update`` takes them."""
        return obs_buf[idx]

    def _rows(self, obs_buf, idx):
        """... as a cond."""
        return {"state": obs_buf[idx].reshape(-1, self.n_cond_step, self.obs_dim)}

    def _apply_gradients(self, st, b, update_actor):
        """What follows minibatch ``b``'s backward; -> whether an optimiser step was taken, so that the call's statistics ``st``
        count.  Here: a step per minibatch."""
        model = self.model
        if self.vf_coef != 1:  # loss = pg + ... + v_loss * vf_coef: the critic sees vf_coef * d v_loss
            model.critic.flat_grads().mul_(self.vf_coef)
        self.dp.allreduce_grads()
        g_lv = sq = None
        if update_actor:
            g_lv = self._logvar_grad(False, 1, not getattr(model, "entropy_in_kernel", False))
        if g_lv is not None and self.max_grad_norm is not None:
            # the reference clips actor_ft.parameters() as ONE group (train_ppo_gaussian_agent.py:319-322), and logvar is
            # one of them: its gradient counts in the norm and is scaled with the trunk's
            sq = self.actor_optimizer.sq_norm(model.actor_ft.flat_grads()).clone() + (g_lv.double() ** 2).sum()
        step_and_repack(model, self.actor_optimizer, self.critic_optimizer, update_actor=update_actor,
                        max_norm=self.max_grad_norm, n_time=None if self._chain_steps() else 0, actor_sq_norm=sq)
        if g_lv is not None:
            self._step_logvar(g_lv, max_norm=self.max_grad_norm, sq_norm=sq)
        return True

    # ------------------------------------------------------------------------------------------------- sample: a chain
    def _policy(self):
        """What the rollout calls per env step: (cond, deterministic, return_chain[, out]) -> Sample."""
        return self.model

    def _old_logprobs(self, cond, chains):
        """The precompute's log-probs of ``n`` buffer rows: (n, Kft, Ta * Da) per chain step here, (n,) for a one-shot sample."""
        n, Kp1, AF = chains.shape
        return self.model.get_logprobs(cond, chains.reshape(n, Kp1, self.horizon_steps, self.action_dim)).reshape(n, Kp1 - 1, AF)

    def _minibatch(self, obs_buf, chains_buf, ret_k, values_buf, adv_k, logp_buf, inds, moments):
        """Loss, backward and device statistics of one minibatch.  Here the model takes the whole buffers plus ``inds`` (the
        others gather first), the critic slice's all-reduce rides the call (ranks > 1), and only here is there a BC term."""
        model, Kft = self.model, self._chain_steps()
        st = model.ppo_update(obs_buf, chains_buf, ret_k, values_buf, adv_k, logp_buf, inds, reward_horizon=self.reward_horizon,
                              global_moments=moments, critic_hook=self.dp.critic_hook)
        if self.use_bc_loss:  # + bc_loss * bc_loss_coeff on the minibatch's observations (reference :329-357)
            rows = torch.div(inds, Kft, rounding_mode="floor")
            model.add_bc_gradient(self._rows(obs_buf, rows), self.bc_loss_coeff / self.world)
        return st

    def _accumulate_logvar(self, first):
        """Behind a minibatch whose gradients are accumulated: a learned std's too."""

    def _logvar_grad(self, accumulated, n_mb, host_entropy):
        """The gradient of a learned std behind ``n_mb`` minibatches, or None where there is none to step."""
        return None

    def _step_logvar(self, g, max_norm=None, sq_norm=None):
        """The learned std's optimiser step with what ``_logvar_grad`` returned (both ``_apply_gradients`` call it behind their
        own step; only a sample axis with a learned std, ``OneShotSample``, has one)."""
        raise NotImplementedError

    def _sample_metrics(self, stats):
        """(the entropy-like term of the logged loss, the record's fields between ``clipfrac`` and ``explained_variance``)."""
        eta = self.model._eta_mean()
        return eta, {"eta": eta}

    # ------------------------------------------------------------------------------------------------- the update
    def _update(self, obs_buf, chains_buf, reward_trajs, terminated_trajs, firsts, last_obs):
        model, dev = self.model, self.device
        S, E = self.n_steps, self.n_envs
        R = S * E
        n_sub = max(self._chain_steps(), 1)  # minibatch entries per buffer row
        self._augment(obs_buf)
        # values and old log-probs over the whole buffer, in logprob_batch_size splits (:203-240)
        values_buf, logp_buf = torch.empty(R, device=dev), None
        for lo in range(0, R, self.logprob_batch_size):
            hi = min(R, lo + self.logprob_batch_size)
            cond = self._rows(obs_buf, slice(lo, hi))
            values_buf[lo:hi] = model.critic(cond, **self.critic_kwargs).reshape(-1)
            lp = self._old_logprobs(cond, chains_buf[lo:hi])
            if logp_buf is None:
                logp_buf = torch.empty((R,) + lp.shape[1:], device=dev)
            logp_buf[lo:hi] = lp
        # running reward scaling on the host, float64 (:243-247)
        if self.reward_scale_running:
            reward_trajs = self.running_reward_scaler(reward=reward_trajs.T, first=firsts[:-1].T).T
        # GAE on the device in float64 (:250-279)
        last_v = model.critic(self._cond(last_obs), **self.critic_kwargs).reshape(-1)
        _, _, adv, ret = gae_device(torch.from_numpy(np.ascontiguousarray(reward_trajs)).to(dev),
                                    values_buf.reshape(S, E), torch.from_numpy(terminated_trajs).float().to(dev),
                                    last_v, self.gamma, self.gae_lambda, self.reward_scale_const)
        adv_k, ret_k = adv.reshape(-1).contiguous(), ret.reshape(-1).contiguous()
        # minibatch PPO (:306-383)
        total = R * n_sub
        num_batch = max(1, total // self.batch_size)
        clipfracs, stats, st, flag_break = [], None, None, False
        update_actor = self.itr >= self.n_critic_warmup_itr
        for _ in range(self.update_epochs):
            perm = torch.randperm(total, device=dev)
            mbs = [perm[b * self.batch_size:(b + 1) * self.batch_size].contiguous() for b in range(num_batch)]
            moments = self.dp.minibatch_moments(adv_k, mbs, n_sub)  # one tiny collective per epoch (None if 1 rank)
            for b, inds in enumerate(mbs):
                st = self._minibatch(obs_buf, chains_buf, ret_k, values_buf, adv_k, logp_buf, inds,
                                     None if moments is None else moments[b])
                if not self._apply_gradients(st, b, update_actor):
                    continue
                stats = st.tolist()  # D2H sync once per optimiser step, as the reference's .item() calls
                clipfracs.append(stats[hip.STAT_CLIPFRAC])
                if (self.target_kl is not None and stats[hip.STAT_APPROX_KL] > self.target_kl
                        and (update_actor or not self.kl_stop_needs_actor)):
                    flag_break = True  # the KL is all-reduced, so every rank takes this branch together
                    break
            if flag_break:
                break
        assert st is not None, "update_epochs must be at least 1"
        if stats is None:  # no optimiser step at all (fewer minibatches than the pixel agents' grad_accumulate): the last call's
            stats = st.tolist()
            clipfracs.append(stats[hip.STAT_CLIPFRAC])
        y_pred, y_true = values_buf.cpu().numpy(), ret_k.cpu().numpy()
        var_y = np.var(y_true)
        ent, fields = self._sample_metrics(stats)
        pg, vl = stats[hip.STAT_PG_LOSS], stats[hip.STAT_V_LOSS]
        return {"loss": pg - ent * self.ent_coef + vl * self.vf_coef, "pg_loss": pg, "v_loss": vl,
                "approx_kl": stats[hip.STAT_APPROX_KL], "ratio": stats[hip.STAT_RATIO],
                "clipfrac": float(np.mean(clipfracs)), **fields,
                "explained_variance": float("nan") if var_y == 0 else float(1 - np.var(y_true - y_pred) / var_y),
                "actor_lr": self.actor_optimizer.param_groups[0]["lr"],
                "critic_lr": self.critic_optimizer.param_groups[0]["lr"]}
