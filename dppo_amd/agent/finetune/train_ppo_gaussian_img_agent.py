"""PPO fine-tuning of a Gaussian policy from pixel observations.  Mirrors the reference's ``TrainPPOImgGaussianAgent``
(agent/finetune/train_ppo_gaussian_img_agent.py): the image agent's observation axis (rollout, augmentation, gradient
accumulation) under the Gaussian arm's sample axis (one action chunk per step, a scalar log-prob, minibatches over R = n_steps *
n_envs rows, a learned per-dimension std stepped with the actor's learning rate)."""
from __future__ import annotations

from dppo_amd.agent.finetune.train_ppo_diffusion_img_agent import TrainPPOImgDiffusionAgent
from dppo_amd.agent.finetune.train_ppo_gaussian_agent import OneShotSample


class TrainPPOImgGaussianAgent(OneShotSample, TrainPPOImgDiffusionAgent):
    pass
