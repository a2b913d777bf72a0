"""Behaviour-cloning pre-training of a Gaussian or mixture-of-Gaussians policy (reference
agent/pretrain/train_gaussian_agent.py:15-101 over train_agent.py:58-168).

The reference's schedule (``PreTrainAgent``) around ``GaussianModel.loss`` / ``GMMModel.loss``: value, entropy and every
gradient of one minibatch come from one library call (dppo_gaussian_bc_loss_fwd_bwd / dppo_gmm_bc_loss_fwd_bwd), the flat
fused AdamW reads the flat gradient the model leaves in ``last_loss_grad``.  A learned std (``logvar``) is not part of the
flat trunk image: it gets its own small AdamW with the same learning rate and weight decay (the reference's one optimiser
covers all ``model.parameters()``), stepped in the same launch, and its own EMA copy.  Checkpoints carry the reference's
state-dict names, so ``GaussianModel(network_path=)`` / ``GMMModel(network_path=)`` and the PPO fine-tuning models load them.
"""
from __future__ import annotations

import logging
import time

import torch

from dppo_amd.agent.pretrain.train_agent import PreTrainAgent
from dppo_amd.util.optim import FlatAdamW, step_many

log = logging.getLogger(__name__)


class TrainGaussianAgent(PreTrainAgent):
    def __init__(self, cfg, dataset=None):
        super().__init__(cfg, dataset)
        self.ent_coef = cfg.train.get("ent_coef", 0)  # entropy bonus (the shipped cfgs leave it at 0)
        self.net.logvar_min.requires_grad_(False)  # the clamp bounds are constants (the base class enabled every parameter)
        self.net.logvar_max.requires_grad_(False)
        self.logvar_optimizer = self.ema_logvar = None
        if getattr(self.net, "learn_fixed_std", False):
            self.logvar_optimizer = FlatAdamW(self.net.logvar.data, lr=cfg.train.learning_rate,
                                              weight_decay=cfg.train.weight_decay)
            self.ema_logvar = self.net.logvar.data.clone()

    def _flat_named_parameters(self):
        inside = {id(p) for p in self.net.trunk_parameters()}  # logvar / logvar_min / logvar_max live outside the flat image
        return [(n, p) for n, p in self.net.named_parameters() if id(p) in inside]

    def step_ema(self):
        super().step_ema()
        if self.ema_logvar is not None:
            lv = self.net.logvar.data
            if self.epoch < self.epoch_start_ema:
                self.ema_logvar.copy_(lv)
            else:
                self.ema_logvar.mul_(self.ema_decay).add_(lv, alpha=1.0 - self.ema_decay)

    def _ema_extra(self):
        return {} if self.ema_logvar is None else {"network.logvar": self.ema_logvar}

    def load(self, epoch):
        data = super().load(epoch)
        if self.ema_logvar is not None:
            self.ema_logvar.copy_(data["ema"]["network.logvar"])
        return data

    def run(self):
        t0 = time.time()
        cnt_batch = 0
        gen = torch.Generator().manual_seed(self.seed)
        history = []
        for _ in range(self.n_epochs):
            losses, ents = [], []
            for batch in self.dataset_train.epoch(self.batch_size, generator=gen):
                loss, info = self.model.loss(batch.actions, batch.conditions, ent_coef=self.ent_coef)
                slots = [self.optimizer.slot(self.model.last_loss_grad)]
                if self.logvar_optimizer is not None:  # same learning rate as the trunk (one optimiser in the reference)
                    self.logvar_optimizer.param_groups[0]["lr"] = self.optimizer.param_groups[0]["lr"]
                    slots.append(self.logvar_optimizer.slot(self.model.last_logvar_grad))
                step_many(slots)
                self.net.mark_updated()
                losses.append(loss.detach())
                ents.append(info["entropy"])
                if cnt_batch % self.update_ema_freq == 0:
                    self.step_ema()
                cnt_batch += 1
            loss_train = float(torch.stack(losses).mean()) if losses else float("nan")
            ent_train = float(torch.stack(ents).mean()) if ents else float("nan")
            self.lr_scheduler.step()
            if self.epoch % self.save_model_freq == 0 or self.epoch == self.n_epochs:
                self.save_model()
            if self.epoch % self.log_freq == 0:
                log.info("%d: train loss %8.4f | entropy: %8.4f | t:%8.4f", self.epoch, loss_train, ent_train, time.time() - t0)
            history.append({"epoch": self.epoch, "loss": loss_train, "entropy": ent_train})
            self.epoch += 1
        self.epoch -= 1
        return history
