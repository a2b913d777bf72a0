"""GPU parity: the HIP path (through the C ABI) vs the reference's golden vectors and the CPU oracle.

Tolerances (stated per SURVEY.md 8c):
  fp32 MFMA path : <= 1e-4 abs/rel on eps / chains / log-probs / losses (exact fp32 products; only the
                   summation order differs from torch's CPU GEMM), <= 2e-4 rel on gradients.
  bf16 MFMA path : operands rounded to bf16 (rel 2^-8), fp32 accumulate: eps <= 3e-2 abs, chains <= 5e-2 abs,
                   log-probs <= 0.6 abs (a 1e-2 error in mu is amplified by z/sigma = 30 at sigma = 0.1) with
                   mean error <= 0.06; loss parity is checked as bitwise self-consistency (ratio == 1) and
                   gradient direction vs the fp32 path (cosine >= 0.99).
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import dppo_oracle as O
from tests.test_oracle_golden import CHAIN_CASES, LOSS_CASES, make_cfg

pytestmark = pytest.mark.gpu

T = torch.from_numpy
DEV = "cuda:0"
HIP_SUPPORTED = {"hopper", "can", "can_relu", "halfcheetah", "kitchen_like", "square_like", "furniture_256", "ln_relu",
                 "transport", "furniture_one_leg"}  # plain (non-residual) MLPs: "next" row


def build_model(sname, kw, seed, precision):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.diffusion_ppo import PPODiffusion
    from dppo_amd.model.diffusion.eta import EtaFixed
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP

    a, c = O.named_specs(sname)
    actor = DiffusionMLP(action_dim=a.action_dim, horizon_steps=a.horizon_steps, cond_dim=a.cond_dim,
                         time_dim=a.time_dim, mlp_dims=list(a.mlp_dims), activation_type=a.activation,
                         cond_mlp_dims=a.cond_mlp_dims, residual_style=True, use_layernorm=a.use_layernorm,
                         precision=precision)
    critic = CriticObs(cond_dim=c.cond_dim, mlp_dims=list(c.mlp_dims), activation_type=c.activation,
                       residual_style=True, use_layernorm=c.use_layernorm, precision=precision)
    actor.load_state_dict(O.init_params(a, seed), strict=True)
    critic.load_state_dict(O.init_params(c, seed + 2), strict=True)
    kw = dict(kw)
    if kw.get("use_ddim"):
        kw["eta"] = EtaFixed(base_eta=1.0)
    kw.setdefault("gamma_denoising", 0.99)
    kw.setdefault("clip_ploss_coef", 0.01)
    m = PPODiffusion(actor=actor, critic=critic, horizon_steps=a.horizon_steps, obs_dim=a.cond_dim,
                     action_dim=a.action_dim, device=DEV, **kw)
    m.actor_ft.load_state_dict(O.init_params(a, seed + 1), strict=True)
    return m, a, c


def test_library_loads_and_versions():
    from dppo_amd import hip
    assert hip.load().dppo_version() == 1


# ------------------------------------------------------------------ G2 network forwards
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 3e-2)])
@pytest.mark.parametrize("name", ["hopper", "can", "can_relu", "halfcheetah", "kitchen_like", "square_like", "furniture_256",
                                  "ln_relu", "transport", "furniture_one_leg"])
def test_network_forward(golden, name, prec, tol):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    g = golden("g2_forward")
    a, c = O.named_specs(name)
    actor = DiffusionMLP(action_dim=a.action_dim, horizon_steps=a.horizon_steps, cond_dim=a.cond_dim,
                         time_dim=a.time_dim, mlp_dims=list(a.mlp_dims), activation_type=a.activation,
                         cond_mlp_dims=a.cond_mlp_dims, residual_style=True, use_layernorm=a.use_layernorm,
                         precision=prec).to(DEV)
    critic = CriticObs(cond_dim=c.cond_dim, mlp_dims=list(c.mlp_dims), activation_type=c.activation,
                       residual_style=True, use_layernorm=c.use_layernorm, precision=prec).to(DEV)
    actor.load_state_dict(O.init_params(a, 11))
    critic.load_state_dict(O.init_params(c, 12))
    st = T(g[f"{name}_state"]).to(DEV)
    eps = actor(T(g[f"{name}_x"]).to(DEV), T(g[f"{name}_t"]).to(DEV), {"state": st})
    val = critic({"state": st})
    np.testing.assert_allclose(eps.cpu().numpy(), g[f"{name}_eps"], rtol=tol, atol=tol)
    np.testing.assert_allclose(val.cpu().numpy(), g[f"{name}_value"], rtol=tol, atol=tol)


def test_forward_ragged_batches():
    """Row-tile edges: batches that are not multiples of the 128/256-row GEMM tiles, incl. a single row."""
    m, a, _ = build_model("hopper", dict(denoising_steps=20, ft_denoising_steps=10), 5, "fp32")
    p = O.init_params(a, 5)
    rs = np.random.RandomState(1)
    for B in (1, 17, 129, 300):
        x = T(rs.randn(B, 4, 3).astype(np.float32))
        t = T(rs.randint(0, 20, size=(B,)).astype(np.int64))
        s = T(rs.uniform(-1, 1, size=(B, 1, 11)).astype(np.float32))
        ref = O.actor_forward(p, a, x, t, s)
        got = m.actor(x.to(DEV), t.to(DEV), {"state": s.to(DEV)})
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------ G3 / G4 chains + log-probs
CHAIN_TOL = {"fp32": dict(chain=1e-4, lp=2e-4, lp_mean=1e-4), "bf16": dict(chain=5e-2, lp=0.6, lp_mean=0.06)}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(k for k, v in CHAIN_CASES.items() if v[0] in HIP_SUPPORTED))
def test_sampling_chain_and_logprobs(golden, case, prec):
    g = golden("g3_chains")
    sname, kw, det = CHAIN_CASES[case]
    m, a, _ = build_model(sname, kw, 21, prec)
    tol = CHAIN_TOL[prec]
    state, noise = T(g[f"{case}_state"]).to(DEV), T(g[f"{case}_noise"]).to(DEV)
    smp = m(cond={"state": state}, deterministic=det, return_chain=True, noise=noise)
    assert tuple(smp.chains.shape) == g[f"{case}_chains"].shape
    np.testing.assert_allclose(smp.chains.cpu().numpy(), g[f"{case}_chains"], rtol=tol["chain"], atol=tol["chain"])
    np.testing.assert_allclose(smp.trajectories.cpu().numpy(), g[f"{case}_traj"], rtol=tol["chain"],
                               atol=tol["chain"])
    lp = m.get_logprobs({"state": state}, T(g[f"{case}_chains"]).to(DEV)).cpu().numpy()
    ref = g[f"{case}_logprobs"]
    # log-probs far in the tail (|z| of 100s under the clipped sigma) are clamped to [-5, 2] downstream
    sel = ref > -50
    np.testing.assert_allclose(lp[sel], ref[sel], rtol=tol["lp"], atol=tol["lp"])
    assert np.abs(lp[sel] - ref[sel]).mean() <= tol["lp_mean"]


def test_sampler_without_chain_and_internal_noise():
    m, a, _ = build_model("hopper", dict(denoising_steps=20, ft_denoising_steps=10, randn_clip_value=3), 3, "bf16")
    st = torch.rand(37, 1, 11, device=DEV) * 2 - 1
    torch.manual_seed(0)
    s1 = m(cond={"state": st}, return_chain=False)
    assert s1.chains is None and tuple(s1.trajectories.shape) == (37, 4, 3)
    torch.manual_seed(0)
    s2 = m(cond={"state": st}, return_chain=True)
    assert torch.equal(s1.trajectories, s2.trajectories)  # same seed, same kernel: bitwise reproducible
    assert torch.equal(s2.chains[:, -1], s2.trajectories)
    assert torch.isfinite(s2.chains).all()


def test_in_kernel_noise_is_standard_normal_and_seeded():
    """Without a noise tensor the sampler draws N(0,1) itself (Philox4x32-10 + Box-Muller): check the moments of x_K
    (chain slot 0 when Kft == K), reproducibility under torch.manual_seed and independence of seeds."""
    m, a, _ = build_model("hopper", dict(denoising_steps=20, ft_denoising_steps=20, randn_clip_value=3), 3, "bf16")
    st = torch.rand(4096, 1, a.cond_dim, device=DEV) * 2 - 1
    torch.manual_seed(123)
    s1 = m(cond={"state": st})
    torch.manual_seed(123)
    s2 = m(cond={"state": st})
    s3 = m(cond={"state": st})
    assert torch.equal(s1.chains, s2.chains) and not torch.equal(s1.chains, s3.chains)
    x = s1.chains[:, 0].double().reshape(-1)  # x_K = the initial draw, unclipped
    n = x.numel()
    assert abs(x.mean().item()) < 4 / n ** 0.5
    assert abs(x.var().item() - 1.0) < 0.03
    assert abs((x ** 4).mean().item() - 3.0) < 0.15
    assert abs((x.abs() > 1.1503).double().mean().item() - 0.25) < 0.01  # P(|z| > 1.1503) = 0.25
    # rows / columns / steps are not correlated with each other
    y = s3.chains[:, 0].double().reshape(-1)
    assert abs((x * y).mean().item()) < 4 / n ** 0.5
    c = s1.chains[:, 0].double()
    assert abs((c[:, 0, 0] * c[:, 1, 1]).mean().item()) < 4 / c.shape[0] ** 0.5


# ------------------------------------------------------------------ G5 PPO loss + gradients
def flat_of(params, spec):
    return np.concatenate([params[n].detach().numpy().reshape(-1) for n, _, _ in O.param_shapes(spec)])


@pytest.mark.parametrize("case", sorted(k for k, v in LOSS_CASES.items() if v[0] in HIP_SUPPORTED))
def test_ppo_loss_and_grads_fp32(golden, case):
    g = golden("g5_loss")
    sname, kw = LOSS_CASES[case]
    m, a, c = build_model(sname, dict(kw, gamma_denoising=0.99, randn_clip_value=3), 31, "fp32")
    d = lambda k: T(g[f"{case}_{k}"]).to(DEV)
    res = m.loss({"state": d("state")}, d("prev"), d("next"), d("kinds"), d("returns"), d("oldvalues"), d("adv"),
                 d("oldlogprobs"), use_bc_loss=False, reward_horizon=int(g[f"{case}_reward_horizon"]))
    stats = g[f"{case}_stats"]
    got = np.array([res[0].item(), float(res[1]), res[2].item(), res[3], res[4], res[5], float(res[6]), res[7]])
    np.testing.assert_allclose(got, stats, rtol=2e-4, atol=2e-5)
    (res[0] + 0.5 * res[2]).backward()
    for mod, tag, scale in ((m.actor_ft, "gactor", 1.0), (m.critic, "gcritic", 0.5)):
        for k, p in mod.named_parameters():
            grad = p.grad.cpu().numpy()
            key = f"{case}_{tag}_{k}"
            ref_n = float(g[key + "__norm"]) if key not in g else float(np.linalg.norm(g[key]))
            atol = 2e-4 * max(ref_n, 1e-8) / np.sqrt(grad.size) + 1e-7
            if key in g:
                np.testing.assert_allclose(grad, g[key], rtol=2e-3, atol=atol)
            else:
                np.testing.assert_allclose(grad.reshape(-1)[::61], g[key + "__sub"], rtol=2e-3, atol=atol)
                assert np.linalg.norm(grad.astype(np.float64)) == pytest.approx(ref_n, rel=2e-4)


def make_rollout(m, a, R, seed):
    """A small synthetic rollout buffer produced by the model itself (device tensors)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
    chains = m(cond={"state": obs}, deterministic=False, return_chain=True).chains
    Kft, AF = m.ft_denoising_steps, a.horizon_steps * a.action_dim
    logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF)
    values = m.critic({"state": obs}).reshape(R)
    returns = values + torch.randn(R, generator=gen).to(DEV) * 0.5
    adv = torch.randn(R, generator=gen).to(DEV) * 2 + 0.3
    return obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), returns, values, adv, logp


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_rollout_mode_matches_oracle_and_is_self_consistent(prec):
    """Fused-gather mode on a rollout buffer: (1) log-probs recomputed inside the loss equal the precomputed
    ones bit for bit (ratio == 1, kl == 0) in BOTH precisions; (2) fp32 statistics and gradients match the CPU
    oracle run on the same gathered minibatch."""
    from dppo_amd import hip
    kw = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, clip_ploss_coef_base=0.001,
              randn_clip_value=3, gamma_denoising=0.99)
    m, a, c = build_model("hopper", kw, 41, prec)
    R, N, Kft = 96, 500, 10
    torch.manual_seed(1)
    obs, chains, returns, values, adv, logp = make_rollout(m, a, R, 7)
    inds = torch.randperm(R * Kft, device=DEV)[:N].contiguous()
    stats = m.ppo_update(obs, chains, returns, values, adv, logp, inds, reward_horizon=4).cpu().numpy()
    assert stats[hip.STAT_RATIO] == pytest.approx(1.0, abs=1e-12)
    assert abs(stats[hip.STAT_APPROX_KL]) <= 1e-12
    assert stats[hip.STAT_CLIPFRAC] == 0.0
    ga = m.actor_ft.flat_grads().cpu().numpy().copy()
    gc = m.critic.flat_grads().cpu().numpy().copy()
    assert np.isfinite(ga).all() and np.isfinite(gc).all()
    # oracle on the gathered minibatch (old log-probs = the HIP path's own, so ratio == 1 there too)
    cfg = make_cfg(a, kw)
    base, ft, cr = O.init_params(a, 41), O.init_params(a, 42), O.init_params(c, 43)
    for p in list(ft.values()) + list(cr.values()):
        p.requires_grad_(True)
    b, k = (inds // Kft).cpu(), (inds % Kft).cpu()
    ch = chains.cpu().reshape(R, Kft + 1, 4, 3)
    res = O.ppo_loss(cfg, a, c, base, ft, cr, obs.cpu().reshape(R, 1, -1)[b], ch[b, k], ch[b, k + 1], k,
                     returns.cpu()[b], values.cpu()[b], adv.cpu()[b], logp.cpu().reshape(R, Kft, 4, 3)[b, k])
    (res[0] + res[2]).backward()
    ref_a, ref_c = flat_of({n: p.grad for n, p in ft.items()}, a), flat_of({n: p.grad for n, p in cr.items()}, c)
    cos = lambda x, y: float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y) + 1e-30))
    if prec == "fp32":
        assert stats[hip.STAT_PG_LOSS] == pytest.approx(res[0].item(), rel=1e-3, abs=1e-5)
        assert stats[hip.STAT_V_LOSS] == pytest.approx(res[2].item(), rel=2e-4)
        # the oracle's ratio deviates from 1 by the fp32 summation-order noise in new log-probs (1e-6), which the
        # 1e-3 clip range turns into a few flipped max() branches: compare direction and norm, not elements
        assert cos(ga, ref_a) >= 0.999 and cos(gc, ref_c) >= 0.9999
        assert np.linalg.norm(gc) == pytest.approx(np.linalg.norm(ref_c), rel=1e-3)
    else:
        assert stats[hip.STAT_V_LOSS] == pytest.approx(res[2].item(), rel=5e-2)
        assert cos(ga, ref_a) >= 0.99 and cos(gc, ref_c) >= 0.99


def test_loss_gathered_equals_rollout_mode():
    """The two input modes of dppo_ppo_loss_fwd_bwd are the same computation."""
    kw = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, randn_clip_value=3)
    m, a, c = build_model("hopper", kw, 51, "fp32")
    R, N, Kft = 64, 256, 10
    torch.manual_seed(2)
    obs, chains, returns, values, adv, logp = make_rollout(m, a, R, 9)
    logp = logp + 0.01 * torch.randn_like(logp)
    inds = torch.randperm(R * Kft, device=DEV)[:N].contiguous()
    s1 = m.ppo_update(obs, chains, returns, values, adv, logp, inds).clone()
    g1 = m.actor_ft.flat_grads().clone()
    b, k = inds // Kft, inds % Kft
    res = m.loss({"state": obs[b].reshape(N, 1, -1)}, chains[b, k].reshape(N, 4, 3), chains[b, k + 1].reshape(N, 4, 3),
                 k, returns[b], values[b], adv[b], logp[b, k].reshape(N, 4, 3))
    assert res[0].item() == pytest.approx(s1[0].item(), rel=1e-6)
    assert torch.allclose(m.actor_ft.flat_grads(), g1, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------ GAE / optimiser
def test_gae_matches_oracle():
    from dppo_amd.util.rollout import gae_device
    rs = np.random.RandomState(3)
    S, E = 50, 37
    r = rs.normal(size=(S, E))
    v = rs.normal(size=(S, E)).astype(np.float32)
    term = (rs.uniform(size=(S, E)) < 0.1).astype(np.float32)
    last = rs.normal(size=(E,)).astype(np.float32)
    adv, ret = O.gae(r, v.astype(np.float64), term.astype(np.float64), last.astype(np.float64), 0.99, 0.95, 0.7)
    a64, r64, a32, r32 = gae_device(T(r).to(DEV), T(v).to(DEV), T(term).to(DEV), T(last).to(DEV), 0.99, 0.95, 0.7)
    np.testing.assert_allclose(a64.cpu().numpy(), adv, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r64.cpu().numpy(), ret, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(a32.cpu().numpy(), adv.astype(np.float32))
    np.testing.assert_array_equal(r32.cpu().numpy(), ret.astype(np.float32))


def test_adamw_and_clip_match_torch(golden):
    from dppo_amd.util.optim import FlatAdamW
    g = golden("g7_adamw")
    p = T(g["p0"].copy()).to(DEV)
    opt = FlatAdamW(p, lr=1e-3, weight_decay=0.01)
    for i in range(3):
        opt.step(T(g[f"g{i}"]).to(DEV))
        np.testing.assert_allclose(p.cpu().numpy(), g[f"p{i + 1}"], rtol=1e-6, atol=1e-7)
    # gradient clipping: one step from zero state with max_norm must equal a step on the clipped gradient
    q1, q2 = torch.zeros(257, device=DEV), torch.zeros(257, device=DEV)
    FlatAdamW(q1, lr=1e-2, weight_decay=0.0).step(T(g["clip_in"]).to(DEV), max_norm=1.5)
    FlatAdamW(q2, lr=1e-2, weight_decay=0.0).step(T(g["clip_out"]).to(DEV))
    np.testing.assert_allclose(q1.cpu().numpy(), q2.cpu().numpy(), rtol=1e-5, atol=1e-8)


def test_adamw_multi_equals_single_steps(golden):
    """dppo_adamw_step_multi (one launch, step count advanced by the slot's last workgroup) == the same steps taken one
    optimiser at a time, bit for bit, over several steps, with clipping on one slot."""
    from dppo_amd.util.optim import FlatAdamW, step_many
    g = golden("g7_adamw")
    gen = torch.Generator(device="cpu").manual_seed(3)
    sizes = (g["p0"].size, 1000, 257)
    ref = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
    ref[0] = T(g["p0"].copy()).to(DEV)
    multi = [r.clone() for r in ref]
    o_ref = [FlatAdamW(p, lr=1e-3 * (i + 1), weight_decay=0.01 * i) for i, p in enumerate(ref)]
    o_mul = [FlatAdamW(p, lr=1e-3 * (i + 1), weight_decay=0.01 * i) for i, p in enumerate(multi)]
    for it in range(4):
        grads = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
        for i, (o, gr) in enumerate(zip(o_ref, grads)):
            o.step(gr, max_norm=0.7 if i == 1 else None)
        step_many([o.slot(gr, max_norm=0.7 if i == 1 else None) for i, (o, gr) in enumerate(zip(o_mul, grads))])
        for a, b, o in zip(ref, multi, o_mul):
            assert torch.equal(a, b)
            assert o._step_dev.tolist() == [it + 1, 0]
    # and the first vector still follows torch.optim.AdamW's trajectory
    p = T(g["p0"].copy()).to(DEV)
    opt = FlatAdamW(p, lr=1e-3, weight_decay=0.01)
    for i in range(3):
        step_many([opt.slot(T(g[f"g{i}"]).to(DEV))])
        np.testing.assert_allclose(p.cpu().numpy(), g[f"p{i + 1}"], rtol=1e-6, atol=1e-7)


def test_denoise_mse_with_100_steps_and_a_32_wide_time_embedding_matches_oracle():
    """K = 100, time_dim = 32 (the furniture cfgs' pre-training): the time MLP's backward block needs 119 KB of LDS, above
    the 64 KB a kernel gets without asking.  fp32 loss and every gradient against the oracle on the same draws."""
    K, N = 100, 48
    m, a, _ = build_model("furniture_256", dict(denoising_steps=K, ft_denoising_steps=10), 81, "fp32")
    for p in m.network.parameters():
        p.requires_grad_(True)
    gen = torch.Generator().manual_seed(9)
    x0 = torch.rand(N, a.horizon_steps, a.action_dim, generator=gen) * 2 - 1
    state = torch.rand(N, 1, a.cond_dim, generator=gen) * 2 - 1
    t = torch.randint(0, K, (N,), generator=gen)
    noise = torch.randn(N, a.horizon_steps, a.action_dim, generator=gen)
    loss = m.p_losses(x0.to(DEV), {"state": state.to(DEV)}, t.to(DEV), noise=noise.to(DEV))
    loss.backward()
    prm = {k: v.clone().requires_grad_(True) for k, v in O.init_params(a, 81).items()}
    ref = O.denoise_mse_loss(K, a, prm, x0, state, t, noise)
    ref.backward()
    assert loss.item() == pytest.approx(ref.item(), rel=1e-4)
    got = torch.cat([p.grad.reshape(-1) for p in m.network.parameters()]).cpu().double().numpy()
    want = flat_of({n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in prm.items()}, a).astype(np.float64)
    assert np.linalg.norm(got - want) <= 2e-4 * np.linalg.norm(want)
    te = slice(0, 32 * 64 + 64 + 64 * 32 + 32)  # the time MLP's parameters come first in the flat layout
    assert np.linalg.norm(want[te]) > 0 and np.linalg.norm(got[te] - want[te]) <= 2e-4 * np.linalg.norm(want[te])


@pytest.mark.parametrize("sname", ["hopper", "square_like", "ln_relu"])
def test_packing_two_networks_at_once_equals_packing_each(sname):
    """dppo_pack_nets (both composites in one launch, both images in one launch) writes byte for byte what two
    dppo_pack_net calls write."""
    from dppo_amd.model.common.mlp import pack_pair
    for prec_name in ("fp32", "bf16"):
        m, a, c = build_model(sname, dict(denoising_steps=20, ft_denoising_steps=10), 71, prec_name)
        K = m.denoising_steps

        def poison():  # invalidate both images; regions a pack does not write (layered-path copies) stay 0xAB either way
            for net in (m.actor_ft, m.critic):
                net.mark_updated()
                for _, buf in net._packed.values():
                    buf.fill_(0xAB)

        m.actor_ft.packed(m.prec, K), m.critic.packed(m.prec, 0)  # allocate
        poison()
        one_a = m.actor_ft.packed(m.prec, K).clone()
        one_c = m.critic.packed(m.prec, 0).clone()
        poison()
        pack_pair(m.critic, 0, m.actor_ft, K, m.prec)
        assert torch.equal(m.actor_ft.packed(m.prec, K), one_a)
        assert torch.equal(m.critic.packed(m.prec, 0), one_c)


def test_stats_travel_through_an_fp32_bucket_without_losing_precision():
    """dppo_stats_split / dppo_stats_merge: float64 statistics as (hi, lo) float32 pairs in the gradient bucket of the
    data-parallel all-reduce; a SUM over `world` identical ranks gives world x the sums and leaves the two advantage
    statistics (global values every rank wrote) unchanged."""
    from dppo_amd import hip
    lib = hip.load()
    st = torch.tensor([-4.76771234567891e-4, 0.506691234567891, 1.50361234567e-5, 7.3167e-2, 0.999861234567891,
                       6.61912345678e-2, 1.02081234567891, 0.0], dtype=torch.float64, device=DEV)
    tail = torch.zeros(16, dtype=torch.float32, device=DEV)
    hip.check(lib.dppo_stats_split(st.data_ptr(), tail.data_ptr(), hip.stream()), "dppo_stats_split")
    assert torch.equal(tail[:8], st.float())
    world = 4
    tail *= world  # what the SUM-reduce over `world` identical ranks leaves (exact: a power of two)
    out = torch.zeros_like(st)
    hip.check(lib.dppo_stats_merge(tail.data_ptr(), out.data_ptr(), world, hip.stream()), "dppo_stats_merge")
    expect = st * world
    expect[5:7] = st[5:7]
    assert torch.allclose(out, expect, rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("case", ["ddim100_5", "ddpm20_ft10"])
def test_logprob_subsample_matches_chain_logprobs(golden, case):
    """get_logprobs_subsample (reference diffusion_vpg.py:398-461) == the matching entries of get_logprobs and of the
    reference's golden log-probs."""
    g = golden("g3_chains")
    sname, kw, _ = CHAIN_CASES[case]
    m, a, _ = build_model(sname, kw, 21, "fp32")
    state = T(g[f"{case}_state"]).to(DEV)
    chains = T(g[f"{case}_chains"]).to(DEV)
    B, Kft = chains.shape[0], m.ft_denoising_steps
    full = m.get_logprobs({"state": state}, chains).reshape(B, Kft, a.horizon_steps, a.action_dim)
    kinds = torch.tensor([(3 * i + 1) % Kft for i in range(B)], device=DEV)
    rows = torch.arange(B, device=DEV)
    sub = m.get_logprobs_subsample({"state": state}, chains[rows, kinds], chains[rows, kinds + 1], kinds)
    np.testing.assert_allclose(sub.cpu().numpy(), full[rows, kinds].cpu().numpy(), rtol=1e-5, atol=1e-5)
    ref = g[f"{case}_logprobs"].reshape(B, Kft, a.horizon_steps, a.action_dim)[rows.cpu().numpy(), kinds.cpu().numpy()]
    sel = ref > -50
    np.testing.assert_allclose(sub.cpu().numpy()[sel], ref[sel], rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("N", [2, 3, 65, 129])
def test_tiny_and_ragged_minibatches_match_oracle(N):
    """Edge sizes of the update: fewer samples than one row tile, one past a tile, ... against the CPU oracle (fp32)."""
    kw = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, randn_clip_value=3)
    m, a, c = build_model("hopper", kw, 9, "fp32")
    cfg = make_cfg(a, kw)
    R, Kft, AF = 40, 10, a.horizon_steps * a.action_dim
    gen = torch.Generator(device="cpu").manual_seed(N)
    obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1)
    chains = m(cond={"state": obs.to(DEV)}).chains.cpu()
    logp = m.get_logprobs({"state": obs.to(DEV)}, chains.to(DEV)).reshape(R, Kft, a.horizon_steps, a.action_dim).cpu()
    ret, val, adv = (torch.randn(R, generator=gen) for _ in range(3))
    inds = torch.randperm(R * Kft, generator=gen)[:N]
    st = m.ppo_update(obs.reshape(R, -1).to(DEV), chains.reshape(R, Kft + 1, AF).to(DEV), ret.to(DEV), val.to(DEV),
                      adv.to(DEV), (logp + 0.01).reshape(R, Kft, AF).to(DEV), inds.to(DEV)).cpu().numpy().copy()
    rows, kk = inds // Kft, inds % Kft
    base, ft, cr = O.init_params(a, 9), O.init_params(a, 10), O.init_params(c, 11)
    ft = {k: v.clone().requires_grad_(True) for k, v in ft.items()}
    cr = {k: v.clone().requires_grad_(True) for k, v in cr.items()}
    res = O.ppo_loss(cfg, a, c, base, ft, cr, obs[rows], chains[rows, kk], chains[rows, kk + 1], kk, ret[rows], val[rows],
                     adv[rows].clone(), logp[rows, kk] + 0.01, reward_horizon=4)
    assert st[0] == pytest.approx(float(res[0].detach()), rel=2e-4, abs=2e-6)
    assert st[1] == pytest.approx(float(res[2].detach()), rel=2e-4, abs=2e-6)
    (res[0] + res[2]).backward()
    ga = torch.cat([ft[k].grad.reshape(-1) if ft[k].grad is not None else torch.zeros(ft[k].numel())
                    for k, _ in m.actor_ft.named_parameters()])
    gc = torch.cat([cr[k].grad.reshape(-1) for k, _ in m.critic.named_parameters()])
    np.testing.assert_allclose(m.actor_ft.flat_grads().cpu().numpy(), ga.numpy(), rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(m.critic.flat_grads().cpu().numpy(), gc.numpy(), rtol=2e-3, atol=2e-6)


def test_sampler_single_env_and_ragged_batches():
    m, a, _ = build_model("hopper", dict(denoising_steps=20, ft_denoising_steps=10, randn_clip_value=3), 3, "fp32")
    base, ft = O.init_params(a, 3), O.init_params(a, 4)
    cfg = make_cfg(a, dict(denoising_steps=20, ft_denoising_steps=10, randn_clip_value=3))
    for B in (1, 15, 17, 33):
        gen = torch.Generator(device="cpu").manual_seed(B)
        st = torch.rand(B, 1, a.cond_dim, generator=gen) * 2 - 1
        noise = torch.randn(21, B, a.horizon_steps, a.action_dim, generator=gen)
        got = m(cond={"state": st.to(DEV)}, noise=noise.to(DEV))
        traj, chains = O.sample_chain(cfg, a, base, ft, st, noise)
        np.testing.assert_allclose(got.chains.cpu().numpy(), chains.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got.trajectories.cpu().numpy(), traj.numpy(), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ G8 behaviour-cloning term
@pytest.mark.parametrize("case", ["bc_ddpm", "bc_ddim_kitchen"])
def test_bc_loss_and_gradient(golden, case):
    """PPODiffusion.loss(use_bc_loss=True)'s BC term (reference diffusion_ppo.py:104-126): value and gradient against
    the reference's golden vectors on the recorded noise (fp32 path), and the autograd hand-off of loss()."""
    from tests.test_oracle_golden import BC_CASES, check_grad
    g = golden("g8_bc")
    sname, kw = BC_CASES[case]
    m, a, _ = build_model(sname, dict(kw, clip_ploss_coef=0.01), 41, "fp32")
    state, noise = T(g[f"{case}_state"]).to(DEV), T(g[f"{case}_noise"]).to(DEV)
    value, grad = m.bc_loss_and_grad({"state": state}, noise=noise)
    assert float(value.item()) == pytest.approx(float(g[f"{case}_bc_loss"]), rel=2e-4, abs=1e-5)
    off = 0
    for k, p in m.actor_ft.named_parameters():
        check_grad(g, f"{case}_gbc_{k}", grad[off:off + p.numel()].view(p.shape).cpu(), 2e-3, 2e-6)
        off += p.numel()
    # accumulation into the PPO gradient
    ga = m.actor_ft.flat_grads()
    ga.fill_(1.0)
    m.add_bc_gradient({"state": state}, 0.5, noise=noise)
    np.testing.assert_allclose(ga.cpu().numpy(), 1.0 + 0.5 * grad.cpu().numpy(), rtol=1e-6, atol=1e-7)


def test_loss_with_bc_term_hands_gradients_to_autograd():
    m, a, c = build_model("hopper", dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01,
                                         randn_clip_value=3), 5, "fp32")
    N, Kft = 32, 10
    gen = torch.Generator(device="cpu").manual_seed(0)
    state = (torch.rand(N, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
    chains = m(cond={"state": state}).chains
    kinds = torch.randint(0, Kft, (N,), generator=gen).to(DEV)
    rows = torch.arange(N, device=DEV)
    oldlp = m.get_logprobs_subsample({"state": state}, chains[rows, kinds], chains[rows, kinds + 1], kinds)
    ret, adv = torch.randn(N, generator=gen).to(DEV), torch.randn(N, generator=gen).to(DEV)
    torch.manual_seed(11)
    res = m.loss({"state": state}, chains[rows, kinds], chains[rows, kinds + 1], kinds, ret, ret.clone(), adv, oldlp,
                 use_bc_loss=True, reward_horizon=4)
    pg, vl, bc = res[0], res[2], res[6]
    assert torch.is_tensor(bc) and bc.requires_grad and math.isfinite(float(bc.detach())) and -2 <= float(bc.detach()) <= 5
    for p in m.actor_ft.parameters():
        p.grad = None
    (pg + 0.5 * vl + 0.25 * bc).backward()
    g_all = torch.cat([p.grad.reshape(-1) for p in m.actor_ft.parameters()])
    expect = m.actor_ft.flat_grads() + 0.25 * m._bc_grad
    np.testing.assert_allclose(g_all.cpu().numpy(), expect.cpu().numpy(), rtol=1e-6, atol=1e-8)


# ------------------------------------------------------------------ fused row-tile kernels vs layered GEMM chain
@pytest.mark.parametrize("case", ["mse_hopper", "mse_can_k100", "mse_can_relu_k100", "mse_square_like", "mse_ln_relu"])
def test_denoise_mse_loss_and_gradients(golden, case):
    """DiffusionModel.p_losses (pre-training loss, reference diffusion.py:325-363) through dppo_denoise_mse_fwd_bwd:
    fp32 against the reference's golden loss and gradients; bf16 against the fp32 result (loss 2e-2, cosine 0.99)."""
    from tests.test_oracle_golden import MSE_CASES
    g = golden("g9_denoise_mse")
    sname, K = MSE_CASES[case]
    d = lambda k: T(g[f"{case}_{k}"]).to(DEV)
    flat = {}
    for prec in ("fp32", "bf16"):
        m, a, _ = build_model(sname, dict(denoising_steps=K, ft_denoising_steps=min(10, K)), 51, prec)
        net = m.network
        for p in net.parameters():  # the fine-tuning wrapper freezes its base policy; pre-training trains it
            p.requires_grad_(True)
        np.testing.assert_allclose(m.q_sample(d("x0"), d("t"), d("noise")).cpu().numpy(), g[f"{case}_xnoisy"], rtol=1e-6,
                                   atol=1e-7)
        loss = m.p_losses(d("x0"), {"state": d("state")}, d("t"), noise=d("noise"))
        loss.backward()
        flat[prec] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).double().cpu().numpy()
        if prec == "fp32":
            assert loss.item() == pytest.approx(float(g[f"{case}_loss"]), rel=1e-4)
            for k, p in net.named_parameters():
                grad, key = p.grad.cpu().numpy(), f"{case}_g_{k}"
                ref_n = float(g[key + "__norm"]) if key not in g else float(np.linalg.norm(g[key]))
                atol = 2e-4 * max(ref_n, 1e-8) / np.sqrt(grad.size) + 1e-7
                if key in g:
                    np.testing.assert_allclose(grad, g[key], rtol=2e-3, atol=atol)
                else:
                    np.testing.assert_allclose(grad.reshape(-1)[::61], g[key + "__sub"], rtol=2e-3, atol=atol)
                    assert np.linalg.norm(grad.astype(np.float64)) == pytest.approx(ref_n, rel=2e-4)
        else:
            assert loss.item() == pytest.approx(float(g[f"{case}_loss"]), rel=2e-2)
    x, y = flat["fp32"], flat["bf16"]
    assert float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y))) >= 0.99
    # the loss draws its own t / noise when none is given, reproducibly under torch.manual_seed
    from dppo_amd.model.diffusion.diffusion import DiffusionModel  # (PPODiffusion.loss is the PPO loss)
    torch.manual_seed(4)
    l1 = DiffusionModel.loss(m, d("x0"), {"state": d("state")}).item()
    torch.manual_seed(4)
    assert DiffusionModel.loss(m, d("x0"), {"state": d("state")}).item() == l1


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("sname", ["hopper", "can", "kitchen_like", "square_like", "transport"])
def test_fused_path_matches_layered_path(prec, tol, sname):
    """Two independent implementations of the big-batch MLP (fused row-tile kernels / layer-by-layer gemm_nt
    chain, tuning knob 1) must agree on log-probs, loss statistics and every gradient."""
    from dppo_amd import hip
    lib = hip.load()
    kw = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, randn_clip_value=3)
    m, a, c = build_model(sname, kw, 71, prec)
    R, N, Kft = 200, 1000, 10  # 200 rows: not a multiple of the 64/32-row tiles
    AF = a.horizon_steps * a.action_dim
    torch.manual_seed(3)
    out = {}
    try:
        for fused in (1, 0):
            lib.dppo_tune_set(1, fused)
            for net in (m.actor, m.actor_ft, m.critic):
                net.mark_updated()  # the packed image depends on the path (layered operands are skipped when fused)
            gen = torch.Generator(device="cpu").manual_seed(5)
            obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
            noise = torch.randn(21, R, AF, generator=gen).to(DEV)
            chains = m(cond={"state": obs}, noise=noise).chains
            logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF)
            val = m.critic({"state": obs}).reshape(R)
            ret = val + torch.randn(R, generator=gen).to(DEV)
            adv = torch.randn(R, generator=gen).to(DEV)
            inds = torch.randperm(R * Kft, generator=gen)[:N].to(DEV).contiguous()
            st = m.ppo_update(obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), ret, val,
                              adv, logp + 0.01, inds).cpu().numpy().copy()
            out[fused] = (logp.cpu().numpy(), val.cpu().numpy(), st, m.actor_ft.flat_grads().cpu().numpy().copy(),
                          m.critic.flat_grads().cpu().numpy().copy())
    finally:
        lib.dppo_tune_set(1, 1)
    lp1, v1, s1, ga1, gc1 = out[1]
    lp0, v0, s0, ga0, gc0 = out[0]
    lp_tol = tol * 30  # d logp = (z / sigma) d mu, sigma >= 0.1
    np.testing.assert_allclose(lp1, lp0, rtol=lp_tol, atol=lp_tol)
    np.testing.assert_allclose(v1, v0, rtol=tol, atol=tol)
    np.testing.assert_allclose(s1[:5], s0[:5], rtol=max(tol * 50, 1e-4), atol=max(tol * 5, 1e-5))
    cos = lambda x, y: float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y) + 1e-30))
    lim = 1 - 1e-6 if prec == "fp32" else 0.995
    assert cos(ga1, ga0) >= lim and cos(gc1, gc0) >= lim
    assert np.linalg.norm(ga1) == pytest.approx(np.linalg.norm(ga0), rel=max(tol * 5, 1e-4))
    assert np.linalg.norm(gc1) == pytest.approx(np.linalg.norm(gc0), rel=max(tol * 5, 1e-4))


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("sname,knob", [("hopper", 22), ("can", 22), ("halfcheetah", 22), ("can_relu", 22), ("hopper", 23),
                                        ("can", 23), ("square_like", 23), ("hopper", 25), ("halfcheetah", 25), ("hopper", 36),
                                        ("can", 36), ("hopper", 37), ("halfcheetah", 37), ("can", 37), ("hopper", 38),
                                        ("hopper", 41), ("hopper", 11), ("hopper", 12), ("hopper", 14), ("hopper", 16),
                                        ("hopper", 18), ("can", 16), ("can", 18)])
def test_one_block_kernels_match_the_general_ones(prec, tol, sname, knob):
    _one_block_ab(prec, tol, sname, knob)


@pytest.mark.parametrize("N,Kft", [(1300, 10), (2100, 10), (6500, 5), (1300, 5), (4103, 7)])
def test_in_kernel_first_layer_gradient_at_other_grids_and_step_counts(N, Kft):
    """Knob 37 beyond the headline shape: minibatches of 21 / 33 / 65 / 102 row tiles (a slab per workgroup: below 32 slabs the
    ordinary reduction, from 32 on the wide one; a last tile with 7 rows), and 5 / 7 fine-tuned steps, where every one-hot column
    fits the 32 (no column is rebuilt from the bias gradient, which then stays the exact fp32 column sum)."""
    _one_block_ab("bf16", 2e-2, "hopper", 37, N=N, Kft=Kft)


def _one_block_ab(prec, tol, sname, knob, N=6500, Kft=10):
    """One-block networks have their own fused kernels.  Knob 22: the forward folds the block's second layer into the out
    layer and the out-layer weight gradient is rebuilt from d_out^T x and d_out^T act(z1) (hopper: actor and critic; halfcheetah
    (24 outputs, ReLU), can (BASELINE configs[2]: 56 outputs, Mish, three input k-steps) and can_relu: the wide-head form, whose
    Wout W2 fragments ride the weight ring, and the critic).  Knob 23: the backward adds dh_1 = d_out . Wout last instead of carrying it,
    in forward-sized tiles, and the second layer's bias gradient comes from colsum(d_out) . Wout (every one-block network
    once the minibatch is large enough for the low-rank dW2).  Knob 25: both walk their short layers without the weight
    stream's padding k-steps (bit-identical arithmetic: the skipped k-steps multiply zeros).  Knob 36: the
    advantage moments as partial sums riding the row builder's launch, added in the loss kernel's prologue.  Knob 37 (bf16): the
    first layer's weight gradient accumulated inside the one-block backward (dh_0 never stored; hopper: actor and critic, the
    others: the critic).  Knob 38: with it, the reductions the backward kernel feeds and the time-embedding gradient on a side
    stream under the weight-gradient GEMMs.  Knob 41: the GEMMs' slab reductions and the post-reduce parts behind them in one
    launch.  Knobs 11, 12, 14, 16, 18: the time-embedding gradient as a pass of its own, one launch per weight-gradient GEMM,
    side streams joined at the call's end, the top block's dW2 as an H x H GEMM (and with it the general backward kernel), the
    post-reduce parts as separate launches -- each of them also takes the in-kernel dW0's conditions away or, for 14, the side
    tail's (csrc/api.hip plan_route(); ``dppo_backward_route`` reports the route).  Same log-probs, values, loss
    statistics and gradients -- tensor by tensor -- as the general kernels."""
    from dppo_amd import hip
    lib = hip.load()
    kw = dict(denoising_steps=20, ft_denoising_steps=Kft, clip_ploss_coef=0.01, randn_clip_value=3)
    m, a, c = build_model(sname, kw, 73, prec)
    R = max(800, -(-N // Kft) + 16)  # (N >= 100 x out_dim: the low-rank dW2 -- and with it the one-block backward -- is on)
    AF = a.horizon_steps * a.action_dim
    out = {}
    default = 0 if knob == 36 else 1  # (ships at 0 = by minibatch size: see csrc/api.hip g_mom_rider)
    try:
        for merged in (1, 0):
            lib.dppo_tune_set(knob, merged if merged or knob != 36 else 2)  # (knob 36: 0 = by minibatch size, 2 = never)
            for net in (m.actor, m.actor_ft, m.critic):
                net.mark_updated()
            gen = torch.Generator(device="cpu").manual_seed(5)
            obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
            chains = (torch.randn(R, Kft + 1, a.horizon_steps, a.action_dim, generator=gen) * 0.5).to(DEV)
            logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF)
            val = m.critic({"state": obs}).reshape(R)
            ret = val + torch.randn(R, generator=gen).to(DEV)
            adv = torch.randn(R, generator=gen).to(DEV)
            inds = torch.randperm(R * Kft, generator=gen)[:N].to(DEV).contiguous()
            st = m.ppo_update(obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), ret, val,
                              adv, logp + 0.01, inds).cpu().numpy().copy()
            grads = {}
            for tag, net in (("a", m.actor_ft), ("c", m.critic)):
                for (k, _), gv in zip(net.named_parameters(), net.grad_views()):
                    grads[(tag, k)] = gv.detach().cpu().numpy().copy()
            out[merged] = (logp.cpu().numpy(), val.cpu().numpy(), st, grads)
    finally:
        lib.dppo_tune_set(knob, default)
        for net in (m.actor, m.actor_ft, m.critic):
            net.mark_updated()
    lp1, v1, s1, g1 = out[1]
    lp0, v0, s0, g0 = out[0]
    np.testing.assert_allclose(lp1, lp0, rtol=tol * 30, atol=tol * 30)
    np.testing.assert_allclose(v1, v0, rtol=tol, atol=tol)
    np.testing.assert_allclose(s1[:5], s0[:5], rtol=max(tol * 50, 1e-4), atol=max(tol * 5, 1e-5))
    for key in g0:  # every tensor: relative L2 error (fp32 1e-4 class; bf16: the operand rounding)
        x, y = g1[key].reshape(-1).astype(np.float64), g0[key].reshape(-1).astype(np.float64)
        err = np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-30)
        assert err <= (2e-4 if prec == "fp32" else 6e-2), (key, err)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("sname", ["can", "kitchen_like", "square_like", "halfcheetah"])
def test_recomputed_logprobs_equal_precomputed_ones_for_every_kernel_family(prec, sname):
    """ratio == 1 and kl == 0 bit for bit with unchanged weights, for the networks the hopper test above does not reach:
    Mish actors (the activation is evaluated by the inference forward without and by the training forward with its
    derivative: both must round the value identically), a cond_mlp encoder, H = 1024, a ReLU actor on the general
    (unmerged) forward."""
    from dppo_amd import hip
    kw = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, clip_ploss_coef_base=0.001,
              randn_clip_value=3, gamma_denoising=0.99)
    m, a, c = build_model(sname, kw, 45, prec)
    R, N, Kft = 96, 700, 10
    AF = a.horizon_steps * a.action_dim
    gen = torch.Generator(device="cpu").manual_seed(9)
    obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
    chains = (torch.randn(R, Kft + 1, a.horizon_steps, a.action_dim, generator=gen) * 0.5).to(DEV)
    logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF).contiguous()
    val = m.critic({"state": obs}).reshape(R)
    ret = val + torch.randn(R, generator=gen).to(DEV)
    adv = torch.randn(R, generator=gen).to(DEV)
    inds = torch.randperm(R * Kft, generator=gen)[:N].to(DEV).contiguous()
    stats = m.ppo_update(obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), ret, val, adv, logp,
                         inds, reward_horizon=a.horizon_steps).cpu().numpy()
    assert stats[hip.STAT_RATIO] == pytest.approx(1.0, abs=1e-12)
    assert abs(stats[hip.STAT_APPROX_KL]) <= 1e-12 and stats[hip.STAT_CLIPFRAC] == 0.0
