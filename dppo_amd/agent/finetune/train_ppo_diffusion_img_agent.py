"""DPPO fine-tuning from pixel observations.  Mirrors ``dppo/agent/finetune/train_ppo_diffusion_img_agent.py`` (reference
``TrainPPOImgDiffusionAgent``): the rollout keeps {"rgb", "state"} per env step, the whole buffer is augmented once per
iteration (random shifts, :188-200), values / log-probs are precomputed in ``logprob_batch_size`` splits, and the update
accumulates the gradients of ``grad_accumulate`` minibatches per optimiser step (:340-372).

What runs where: both ViT encoders, the denoiser, the critic, the loss and all gradients are the HIP library's
(``dppo_vis_*`` + the ``*_obs`` loss entries); each network has two flat parameter buffers (encoder, trunk) and the four
gradient accumulators of a step are slices of ONE bucket, which is also the data-parallel all-reduce payload.

The iteration and the update's skeleton are ``TrainPPODiffusionAgent``'s; this class is the observation axis for pixels (the
rollout, the augmentation, how rows become a cond, gradient accumulation) and the chain's minibatch call on gathered rows.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from dppo_amd import hip
from dppo_amd.agent.finetune.train_ppo_diffusion_agent import TrainPPODiffusionAgent
from dppo_amd.model.common.modules import RandomShiftsAug
from dppo_amd.util.optim import FlatAdamW, step_many
from dppo_amd.util.rollout import stack_obs


class TrainPPOImgDiffusionAgent(TrainPPODiffusionAgent):
    kl_stop_needs_actor = True  # (the state agents stop on the KL during the critic warm-up too)
    critic_kwargs = {"no_augment": True}  # the buffer was augmented once, in front of the precompute

    def __init__(self, cfg, venv=None):
        super().__init__(cfg, venv=venv)
        model = self.model
        if not getattr(model.actor_ft, "is_vision", False) or not getattr(model.critic, "is_vision", False):
            raise TypeError("TrainPPOImgDiffusionAgent needs pixel networks (VisionDiffusionMLP / VisionUnet1D + ViTCritic)")
        self.augment = cfg.train.get("augment", False)
        if self.augment:
            self.aug = RandomShiftsAug(pad=4)
        shape_meta = cfg.shape_meta
        self.obs_dims = {k: list(shape_meta.obs[k]["shape"]) for k in shape_meta.obs}
        self.grad_accumulate = cfg.train.get("grad_accumulate", 1)
        if self.use_bc_loss:
            raise NotImplementedError("dppo_amd: the BC term with pixel networks is not built")
        a, c = model.actor_ft, model.critic
        if self.world > 1:  # the parent broadcast the trunks; the encoders too
            for net in (a, c, model.actor):
                dist.broadcast(net.vis.flat_params(), src=0)
                net.vis.mark_updated()
        # the encoders step with their network's hyper-parameters and learning-rate schedule (one param group in the reference)
        self.actor_vis_optimizer = FlatAdamW(a.vis.flat_params(), lr=cfg.train.actor_lr, weight_decay=cfg.train.actor_weight_decay)
        self.critic_vis_optimizer = FlatAdamW(c.vis.flat_params(), lr=cfg.train.critic_lr, weight_decay=cfg.train.critic_weight_decay)
        self.actor_vis_optimizer.param_groups = self.actor_optimizer.param_groups
        self.critic_vis_optimizer.param_groups = self.critic_optimizer.param_groups
        # accumulators: [actor trunk | actor encoder | critic trunk | critic encoder] in one bucket
        sizes = [a.flat_params().numel(), a.vis.flat_params().numel(), c.flat_params().numel(), c.vis.flat_params().numel()]
        self._bucket = torch.zeros(sum(sizes), dtype=torch.float32, device=self.device)
        offs = np.cumsum([0] + sizes)
        self._acc = [self._bucket[offs[i]:offs[i + 1]] for i in range(4)]
        self._norm = torch.zeros(1, dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------------------------------------- rollout
    def _cond(self, obs):
        return {k: torch.from_numpy(obs[k]).to(self.device, non_blocking=True) for k in self.obs_dims}

    def _collect(self, prev_obs, eval_mode):
        """A plain step loop: the whole observation dict crosses to the device, the sampler runs, the envs step."""
        S, E, Kft = self.n_steps, self.n_envs, self._chain_steps()
        R, AF = S * E, self.horizon_steps * self.action_dim
        if self._bufs is None:  # images in the dtype the env hands over (uint8 stays uint8)
            self._bufs = ({k: torch.empty((R,) + tuple(prev_obs[k].shape[1:]), device=self.device,
                                          dtype=torch.uint8 if prev_obs[k].dtype == np.uint8 else torch.float32)
                           for k in self.obs_dims}, torch.empty(R, Kft + 1, AF, device=self.device))
        bufs, chains_buf = self._bufs
        policy = self._policy()
        reward_trajs, terminated_trajs, done_trajs = np.zeros((S, E)), np.zeros((S, E)), np.zeros((S, E))
        for step in range(S):
            cond = self._cond(prev_obs)
            for k in bufs:
                bufs[k][step * E:(step + 1) * E] = cond[k]
            smp = policy(cond=cond, deterministic=eval_mode, return_chain=True)
            chains_buf[step * E:(step + 1) * E] = smp.chains.reshape(E, Kft + 1, AF)
            action = smp.trajectories.cpu().numpy()[:, :self.act_steps]
            prev_obs, reward, terminated, truncated, _ = self.venv.step(action)
            prev_obs = stack_obs(prev_obs)
            reward_trajs[step], terminated_trajs[step], done_trajs[step] = reward, terminated, terminated | truncated
        return reward_trajs, terminated_trajs, done_trajs, prev_obs

    # ------------------------------------------------------------------------------------------------- update
    def _augment(self, bufs):
        """One random shift per stored image, before anything reads the buffer (reference :188-200)."""
        if not self.augment:
            return
        rgb = bufs["rgb"]
        dt = rgb.dtype
        for lo in range(0, rgb.shape[0], 4096):
            x = rgb[lo:lo + 4096]
            y = self.aug(x.reshape(-1, *x.shape[2:]))  # "(s e t) c h w": every frame of the history shifts on its own
            rgb[lo:lo + 4096] = y.reshape(x.shape).to(dt)

    def _gather(self, bufs, idx):
        return {k: bufs[k][idx] for k in bufs}

    _rows = _gather

    def _grad_bufs(self):
        a, c = self.model.actor_ft, self.model.critic
        return [a.flat_grads(), a.vis.flat_grads(), c.flat_grads(), c.vis.flat_grads()]

    def _accumulate(self, first: bool):
        lib = hip.load()
        for acc, g, scale in zip(self._acc, self._grad_bufs(), (1.0, 1.0, self.vf_coef, self.vf_coef)):
            if first:
                acc.copy_(g)
                if scale != 1.0:
                    acc.mul_(scale)
            else:
                hip.check(lib.dppo_axpy(acc.data_ptr(), g.data_ptr(), float(scale), acc.numel(), hip.stream()), "dppo_axpy")

    def _optimizer_step(self, update_actor: bool):
        """One AdamW launch over the four accumulators; the actor's clip norm spans its trunk and its encoder
        (clip_grad_norm_ over actor_ft.parameters(), reference :347-351)."""
        model = self.model
        if self.world > 1:
            dist.all_reduce(self._bucket)
        slots = [self.critic_optimizer.slot(self._acc[2]), self.critic_vis_optimizer.slot(self._acc[3])]
        if update_actor:
            norm = None
            if self.max_grad_norm is not None:
                n1 = self.actor_optimizer.sq_norm(self._acc[0]).clone()
                n2 = self.actor_vis_optimizer.sq_norm(self._acc[1])
                self._norm.copy_(n1 + n2)
                norm = self._norm
            slots += [self.actor_optimizer.slot(self._acc[0], max_norm=self.max_grad_norm, sq_norm=norm),
                      self.actor_vis_optimizer.slot(self._acc[1], max_norm=self.max_grad_norm, sq_norm=norm)]
        step_many(slots)
        model.critic.mark_updated()
        if update_actor:
            model.actor_ft.mark_updated()

    def _apply_gradients(self, st, b, update_actor):
        """Accumulate; every ``grad_accumulate`` minibatches of an epoch one optimiser step (none at all with fewer minibatches
        than that; what is left over at an epoch's end is dropped), behind it the statistics' all-reduce."""
        n = self.grad_accumulate
        self._accumulate(first=b % n == 0)
        self._accumulate_logvar(first=b % n == 0)
        if (b + 1) % n != 0:
            return False
        self._optimizer_step(update_actor)
        g_lv = self._logvar_grad(True, n, True) if update_actor else None
        if g_lv is not None:  # (unclipped, and the entropy term of all n minibatches: open)
            self._step_logvar(g_lv)
        if self.world > 1:
            dist.all_reduce(st)
            st[5:7] /= self.world
        return True

    def _minibatch(self, bufs, chains_buf, ret_k, values_buf, adv_k, logp_buf, inds, moments):
        model, Kft = self.model, self._chain_steps()
        quant = (model.clip_advantage_lower_quantile, model.clip_advantage_upper_quantile) != (0, 1)
        rows = torch.div(inds, Kft, rounding_mode="floor")
        kinds = inds - rows * Kft
        cond = self._gather(bufs, rows)
        pairs = torch.stack([chains_buf[rows, kinds], chains_buf[rows, kinds + 1]], dim=1).contiguous()
        adv_b = adv_k[rows].contiguous()
        return model._run_ppo_vision(cond, pairs, ret_k[rows].contiguous(), values_buf[rows].contiguous(),
                                     adv_b, logp_buf[rows, kinds].contiguous(), kinds.contiguous(), inds.numel(),
                                     self.reward_horizon, adv_b if quant else None, moments)
