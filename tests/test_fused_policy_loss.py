"""The policy half of the PPO loss inside the actor's fused forward (tuning knob 42; csrc/loss_dev.h, csrc/fused.hip LOSSF).

Every case runs ``ppo_update`` twice from identical inputs and zeroed gradient buffers -- knob 42 on, knob 42 off -- and the
statistics and both networks' flat gradients must be equal BIT FOR BIT: the fused epilogue does the loss kernel's arithmetic
in the loss kernel's order, only spread over the workgroup.  ``dppo_ppo_loss_route`` says which of the two the knob-on run took,
and the inputs are built so that the equality says something: the actor's weights are perturbed after the old log-probs were
recorded (ratio != 1), a quarter of the rollout rows have every x_{k+1} many std_k away from the posterior mean (both log-probs
clamp at -5: ratio == 1 exactly, never clipped), another quarter have half of their elements there (the clamp mask inside a
row), and the rest are clipped or not as the perturbation has it -- except rows 2 mod 4, whose recorded log-probs are lowered
by 0.5 as well, which puts their ratio outside every clip range whatever the perturbation does (0 < clipfrac < 1 even at N = 2).

Shapes: hopper's networks (H 512 actor, H 256 critic, Kft 10) on a rollout of 8 envs x 40 steps; N = 2 / 64 / 65 / 255 (one
tile, a full tile, a tile and one sample, four tiles with a ragged last one) and 16,449 (258 tiles: more than there are CUs, so
some workgroups walk a second tile, and the last tile holds one sample).  Below 16,385 samples the advantage moments would ride
the row builder, which the fused route leaves to the loss launch: those cases set knob 36 = 2."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import dppo_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KFT, ENVS, STEPS = 10, 8, 40
R = ENVS * STEPS


def _env_knob(knob, default):
    env = dict(kv.split("=") for kv in filter(None, os.environ.get("DPPO_TUNE", "").split(",")))
    return int(env.get(str(knob), default))


@pytest.fixture(autouse=True)
def knobs_back():
    """Whatever a test sets, the next one starts from the suite's knobs (the suite is also run with DPPO_TUNE=42=0)."""
    from dppo_amd import hip
    yield
    lib = hip.load()
    for knob, default in ((42, 1), (36, 0), (2, 1)):
        lib.dppo_tune_set(knob, _env_knob(knob, default))


def build(actor_spec, critic_spec, prec, norm_adv, seed=61):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.diffusion_ppo import PPODiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP

    a, c = actor_spec, critic_spec
    actor = DiffusionMLP(action_dim=a.action_dim, horizon_steps=a.horizon_steps, cond_dim=a.cond_dim, time_dim=a.time_dim,
                         mlp_dims=list(a.mlp_dims), activation_type=a.activation, cond_mlp_dims=a.cond_mlp_dims,
                         residual_style=True, use_layernorm=a.use_layernorm, precision=prec)
    critic = CriticObs(cond_dim=c.cond_dim, mlp_dims=list(c.mlp_dims), activation_type=c.activation, residual_style=True,
                       use_layernorm=c.use_layernorm, precision=prec)
    actor.load_state_dict(O.init_params(a, seed), strict=True)
    critic.load_state_dict(O.init_params(c, seed + 2), strict=True)
    m = PPODiffusion(actor=actor, critic=critic, horizon_steps=a.horizon_steps, obs_dim=a.cond_dim, action_dim=a.action_dim,
                     device=DEV, denoising_steps=20, ft_denoising_steps=KFT, randn_clip_value=3, gamma_denoising=0.99,
                     clip_ploss_coef=0.01, clip_ploss_coef_base=0.001, norm_adv=norm_adv, clip_advantage_lower_quantile=0.05,
                     clip_advantage_upper_quantile=0.95)
    m.actor_ft.load_state_dict(O.init_params(a, seed + 1), strict=True)
    return m


def rollout(m, a, seed=17):
    """The rollout buffer: chains sampled by the model, then rows 1 mod 4 moved far from every posterior mean (consecutive chain
    positions 16 apart), rows 3 mod 4 in the first half of their elements only; old log-probs recorded on THESE chains (rows 2 mod
    4: lowered by 0.5), and the fine-tuned actor's weights perturbed afterwards."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    AF = a.horizon_steps * a.action_dim
    obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
    torch.manual_seed(seed)
    chains = m(cond={"state": obs}, deterministic=False, return_chain=True).chains.reshape(R, KFT + 1, AF).clone()
    sign = (8.0 * (-1.0) ** torch.arange(KFT + 1, device=DEV)).reshape(1, KFT + 1, 1)
    chains[1::4] += sign
    chains[3::4, :, :AF // 2] += sign
    logp = m.get_logprobs({"state": obs}, chains.reshape(R, KFT + 1, a.horizon_steps, a.action_dim)).reshape(R, KFT, AF).contiguous()
    logp[2::4] -= 0.5
    values = m.critic({"state": obs}).reshape(R)
    returns = values + torch.randn(R, generator=gen).to(DEV) * 0.5
    adv = torch.randn(R, generator=gen).to(DEV) * 2 + 0.3
    with torch.no_grad():
        for p in m.actor_ft.parameters():
            p.mul_(1 + 0.2 * torch.randn(p.shape, generator=gen).to(DEV))
    m.actor_ft.mark_updated()
    return obs.reshape(R, -1).contiguous(), chains.contiguous(), returns, values, adv, logp


def sample_inds(N, seed=3):
    """N (rollout row, step) pairs; the first two are a far row and an ordinary one, so that even N = 2 has both kinds."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    inds = torch.randint(0, R * KFT, (N,), generator=gen)
    inds[0], inds[1] = 1 * KFT + 4, 2 * KFT + 7
    return inds.to(DEV).contiguous()


def update(m, data, inds, mode, rh, gm):
    obs, chains, returns, values, adv, logp = data
    for net in (m.actor_ft, m.critic):
        net.flat_grads().zero_()
    if mode == "rollout":
        st = m.ppo_update(obs, chains, returns, values, adv, logp, inds, reward_horizon=rh, global_moments=gm)
    else:  # the minibatch gathered on the host side: one row per sample, its denoising step in ``kinds``
        N = inds.numel()
        b, k = inds // KFT, inds % KFT
        pairs = torch.stack([chains[b, k], chains[b, k + 1]], dim=1).contiguous()
        st = m._run_ppo(obs[b].contiguous(), pairs, returns[b].contiguous(), values[b].contiguous(), adv[b].contiguous(),
                        logp[b, k].contiguous(), None, k.contiguous(), N, rh, adv[b], gm)
    torch.cuda.synchronize()
    return (st.cpu().numpy().copy(), m.actor_ft.flat_grads().cpu().numpy().copy(), m.critic.flat_grads().cpu().numpy().copy())


def moments_of(adv, inds):
    am = adv[inds // KFT].double()
    return torch.stack([am.sum(), (am * am).sum(), torch.tensor(float(inds.numel()), dtype=torch.float64, device=DEV)])


def route(m, N, gm):
    from dppo_amd import hip
    da, dc = m.actor_ft.net_desc(), m.critic.net_desc()
    rc = hip.load().dppo_ppo_loss_route(C.byref(da), C.byref(dc), m.prec, N, int(gm is not None))
    assert rc in (0, 1), hip.load().dppo_last_error()
    return rc


def on_and_off(m, data, inds, mode, rh, gm, expect_fused):
    """The update with knob 42 on and off; returns the knob-off statistics."""
    from dppo_amd import hip
    lib = hip.load()
    N = inds.numel()
    assert lib.dppo_tune_set(42, 1) == 0
    assert route(m, N, gm) == (1 if expect_fused else 0)
    on = update(m, data, inds, mode, rh, gm)
    assert lib.dppo_tune_set(42, 0) == 0
    assert route(m, N, gm) == 0
    off = update(m, data, inds, mode, rh, gm)
    for name, x, y in zip(("stats", "actor gradients", "critic gradients"), on, off):
        assert np.isfinite(y).all(), name
        bits = np.int64 if x.dtype == np.float64 else np.int32
        diff = x.view(bits) != y.view(bits)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} words differ, first at {int(np.argmax(diff))}"
    assert np.abs(off[1]).max() > 0 and np.abs(off[2]).max() > 0
    return off[0]


# (N, activation, mode, norm_adv, reward_horizon, global moments given)
CASES = [
    (2, "ReLU", "rollout", True, 4, False),
    (2, "Mish", "gathered", False, 2, True),
    (64, "ReLU", "gathered", True, 4, True),
    (64, "Mish", "rollout", False, 4, False),
    (65, "Mish", "rollout", False, 2, False),
    (65, "ReLU", "gathered", True, 2, True),
    (255, "ReLU", "rollout", True, 2, True),
    (255, "Mish", "gathered", True, 4, False),
    (255, "ReLU", "gathered", False, 4, False),
    (16449, "ReLU", "rollout", True, 4, False),
    (16449, "Mish", "gathered", False, 2, False),
    (16449, "ReLU", "rollout", True, 2, True),
]


@pytest.mark.parametrize("N,act,mode,norm_adv,rh,with_gm", CASES)
def test_fused_policy_loss_equals_the_loss_launch_bit_for_bit(N, act, mode, norm_adv, rh, with_gm):
    from dppo_amd import hip
    a, c = O.named_specs("hopper")
    a = dataclasses.replace(a, activation=act)
    m = build(a, c, "bf16", norm_adv)
    data = rollout(m, a)
    inds = sample_inds(N)
    gm = moments_of(data[4], inds) if with_gm else None
    if N <= 16384:  # (the 16,449 cases run with default knobs)
        assert hip.load().dppo_tune_set(36, 2) == 0
    st = on_and_off(m, data, inds, mode, rh, gm, expect_fused=True)
    # the equality above is about something: the recomputed log-probs differ from the recorded ones, and the clipped surrogate
    # takes both branches
    assert st[hip.STAT_RATIO] != 1.0
    assert 0.0 < st[hip.STAT_CLIPFRAC] < 1.0


@pytest.mark.parametrize("what", ["fp32", "24 outputs", "riders", "one stream"])
def test_everything_else_keeps_the_loss_launch(what):
    """The route query answers "separate" for fp32, an actor with 24 outputs (halfcheetah's), a minibatch whose advantage moments
    ride the row builder (N = 4,096, default knobs) and the value half on the actor's stream (knob 2 = 0) -- and there the knob
    changes nothing."""
    from dppo_amd import hip
    lib = hip.load()
    a, c = O.named_specs("halfcheetah" if what == "24 outputs" else "hopper")
    m = build(a, c, "fp32" if what == "fp32" else "bf16", True)
    data = rollout(m, a)
    N = 4096 if what == "riders" else 255
    inds = sample_inds(N)
    if what != "riders":
        assert lib.dppo_tune_set(36, 2) == 0
    if what == "one stream":
        assert lib.dppo_tune_set(2, 0) == 0
    on_and_off(m, data, inds, "rollout", 4, None, expect_fused=False)
