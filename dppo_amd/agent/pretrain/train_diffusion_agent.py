"""Pre-training of a diffusion policy (reference agent/pretrain/train_agent.py:58-168, train_diffusion_agent.py:18-88).

Same schedule as the reference -- AdamW, cosine LR with warm-up per epoch, EMA copy updated every ``update_ema_freq``
batches once ``epoch_start_ema`` is reached, checkpoints {"epoch", "model", "ema"} that ``DiffusionModel(network_path=)``
and the fine-tuning agents load -- on the HIP path: the supervised loss and all its gradients come from
``DiffusionModel.loss`` (dppo_denoise_mse_fwd_bwd), the optimiser is the flat fused AdamW, the EMA is one fused
multiply-add over the flat parameter image, minibatches are gathered on the device (all but ``run`` lives in
``PreTrainAgent``, train_agent.py).
"""
from __future__ import annotations

import logging
import time

import torch

from dppo_amd.agent.pretrain.train_agent import PreTrainAgent
from dppo_amd.util.optim import step_many

log = logging.getLogger(__name__)


class TrainDiffusionAgent(PreTrainAgent):
    def run(self):
        t0 = time.time()
        cnt_batch = 0
        gen = torch.Generator().manual_seed(self.seed)
        history = []
        for _ in range(self.n_epochs):
            losses = []
            for batch in self.dataset_train.epoch(self.batch_size, generator=gen):
                # value + every gradient in one library call; `loss.backward()` would hand each parameter its slice of the
                # same flat image (that is what a torch optimiser needs) -- the flat AdamW reads it directly
                loss = self.model.loss(batch.actions, batch.conditions)
                step_many([self.optimizer.slot(self.model.last_loss_grad)])
                self.net.mark_updated()
                losses.append(loss.detach())
                if cnt_batch % self.update_ema_freq == 0:
                    self.step_ema()
                cnt_batch += 1
            loss_train = float(torch.stack(losses).mean()) if losses else float("nan")
            self.lr_scheduler.step()
            if self.epoch % self.save_model_freq == 0 or self.epoch == self.n_epochs:
                self.save_model()
            if self.epoch % self.log_freq == 0:
                log.info("%d: train loss %8.4f | t:%8.4f", self.epoch, loss_train, time.time() - t0)
            history.append({"epoch": self.epoch, "loss": loss_train})
            self.epoch += 1
        self.epoch -= 1
        return history
