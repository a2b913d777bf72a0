"""What every pre-training agent shares (reference agent/pretrain/train_agent.py:58-168, ``PreTrainAgent``): seeding, the
model from the cfg, AdamW with the cosine warm-up schedule stepped per epoch, the EMA copy updated every ``update_ema_freq``
batches once ``epoch_start_ema`` is reached, and checkpoints {"epoch", "model", "ema"} in the reference's state-dict names.

On the HIP path the optimiser is the flat fused AdamW over the network's flat parameter image, the EMA is one fused
multiply-add over that image, and minibatches are gathered on the device.  Subclasses write ``run()`` around their model's
``loss`` (which leaves the flat gradient in ``model.last_loss_grad``).
"""
from __future__ import annotations

import logging
import os
import random

import numpy as np
import torch

from dppo_amd.cfg.loader import instantiate
from dppo_amd.util.optim import FlatAdamW
from dppo_amd.util.scheduler import CosineAnnealingWarmupRestarts

log = logging.getLogger(__name__)


class PreTrainAgent:
    def __init__(self, cfg, dataset=None):
        self.cfg = cfg
        self.seed = cfg.get("seed", 42)
        random.seed(self.seed)
        np.random.seed(self.seed)
        torch.manual_seed(self.seed)
        self.model = instantiate(cfg.model)
        self.net = self.model.network
        for p in self.net.parameters():
            p.requires_grad_(True)
        self.ema_decay = cfg.ema.decay
        self.ema_flat = self.net.flat_params().clone()  # reset_parameters(): the EMA starts as a copy of the model
        self.n_epochs, self.batch_size = cfg.train.n_epochs, cfg.train.batch_size
        self.epoch_start_ema = cfg.train.get("epoch_start_ema", 20)
        self.update_ema_freq = cfg.train.get("update_ema_freq", 10)
        self.logdir = cfg.logdir
        self.checkpoint_dir = os.path.join(self.logdir, "checkpoint")
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.log_freq = cfg.train.get("log_freq", 1)
        self.save_model_freq = cfg.train.save_model_freq
        self.dataset_train = dataset if dataset is not None else instantiate(cfg.train_dataset)
        self.optimizer = FlatAdamW(self.net.flat_params(), lr=cfg.train.learning_rate,
                                   weight_decay=cfg.train.weight_decay)
        sch = cfg.train.lr_scheduler
        self.lr_scheduler = CosineAnnealingWarmupRestarts(
            self.optimizer, first_cycle_steps=sch.first_cycle_steps, cycle_mult=1.0, max_lr=cfg.train.learning_rate,
            min_lr=sch.min_lr, warmup_steps=sch.warmup_steps, gamma=1.0)
        self.epoch = 1

    # ---- EMA (train_agent.py:36-56, :137-144)
    def step_ema(self):
        p = self.net.flat_params()
        if self.epoch < self.epoch_start_ema:
            self.ema_flat.copy_(p)
        else:
            self.ema_flat.mul_(self.ema_decay).add_(p, alpha=1.0 - self.ema_decay)

    def _ema_extra(self):
        """EMA copies of the parameters outside the flat image, by state-dict key (none here)."""
        return {}

    def _state_dict_of(self, flat, extra=None):
        """state_dict of the whole model with the network's flat-image parameters taken from ``flat`` (and those in
        ``extra`` from there)."""
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        off = 0
        for name, p in self._flat_named_parameters():
            sd["network." + name] = flat[off:off + p.numel()].view(p.shape).detach().clone()
            off += p.numel()
        for k, v in (extra or {}).items():
            sd[k] = v.detach().clone()
        return sd

    def _flat_named_parameters(self):
        """(name, parameter) of the parameters the flat image covers, in its order (here: all of the network's)."""
        return list(self.net.named_parameters())

    def save_model(self):
        path = os.path.join(self.checkpoint_dir, f"state_{self.epoch}.pt")
        torch.save({"epoch": self.epoch, "model": self._state_dict_of(self.net.flat_params()),
                    "ema": self._state_dict_of(self.ema_flat, self._ema_extra())}, path)
        log.info("Saved model to %s", path)
        return path

    def load(self, epoch):
        data = torch.load(os.path.join(self.checkpoint_dir, f"state_{epoch}.pt"), weights_only=True)
        self.epoch = data["epoch"]
        self.model.load_state_dict(data["model"])
        self.net.mark_updated()
        off, flat = 0, self.ema_flat
        for name, p in self._flat_named_parameters():
            flat[off:off + p.numel()].copy_(data["ema"]["network." + name].reshape(-1))
            off += p.numel()
        return data

    def run(self):
        raise NotImplementedError
