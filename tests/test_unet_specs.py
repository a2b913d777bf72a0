"""The conv denoiser (dppo_unet_*, csrc/unet.hip) over the descriptor space check_desc accepts, not just the shipped shapes:
one to four levels, widths that are no multiple of 64, T from 1 to 64, one channel per group, decreasing multipliers (an
identity skip that reads a split concat image), action_dim == dim.  The HIP path runs against the oracle evaluated in
float64 on the CPU inside the test (no fixtures); two CPU tests keep the bounds honest (oracle float32 vs float64 to a tenth
of every fp32 bound) and the state-dict order right.  Bounds are those of tests/test_unet.py."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import dppo_oracle as O
from tests.test_oracle_golden import make_cfg
from tests.test_unet import CRITIC, grad_report, hip_unet

EDGE_SPECS = {
    # one channel per group, 2-element groups (cnt < 64 lanes), Da = cond = 1, time_dim 4
    "tiny_cg1": dict(dim=8, dim_mults=(1, 2), n_groups=8, horizon_steps=2, action_dim=1, cond_dim=1, diffusion_step_embed_dim=4,
                     kernel_size=3),
    # one level (no down / up / concat), T = 1, GroupNorm with one group
    "l1_t1": dict(dim=8, dim_mults=(1,), n_groups=1, horizon_steps=1, kernel_size=3, action_dim=3, cond_dim=5),
    # odd horizon, 72 channels (padded to 128), 9 groups
    "odd_t3": dict(dim=72, dim_mults=(1,), n_groups=9, horizon_steps=3, kernel_size=3, action_dim=5, cond_dim=7),
    # the constructor default: four levels, T 8 -> 1, every cat[l] in use
    "l4_default": dict(dim=32, dim_mults=(1, 2, 4, 8), diffusion_step_embed_dim=32, horizon_steps=8, action_dim=7, cond_dim=23),
    # four levels with widths 24 / 48 / 72 / 96, additive FiLM, ReLU, cond_dim > 64
    "l4_t16_k3": dict(dim=24, dim_mults=(1, 2, 3, 4), kernel_size=3, n_groups=4, cond_predict_scale=False, activation="ReLU",
                      horizon_steps=16, cond_dim=70, action_dim=4),
    # identity skip through a split concat image, halves of 40 (up_modules.0.0: 2 * 40 -> 80)
    "dec_40": dict(dim=40, dim_mults=(1, 2, 1), horizon_steps=4, action_dim=7, cond_dim=23),
    # the same with halves of 64 (the aligned case), additive FiLM, k 3
    "dec_32": dict(dim=32, dim_mults=(1, 4, 2), horizon_steps=8, kernel_size=3, cond_predict_scale=False, action_dim=6, cond_dim=11),
    # action_dim == dim == 64: identity skip in down_modules.0.0, first conv without channel padding, Kg = 320, 32 groups
    "flat_64": dict(action_dim=64, dim=64, dim_mults=(1, 1), n_groups=32, diffusion_step_embed_dim=128, cond_dim=130,
                    horizon_steps=2),
    # widths 136 / 272 (padded to 192 / 320), T = 6 -> 3
    "wide_136": dict(dim=136, dim_mults=(1, 2), horizon_steps=6, action_dim=3, cond_dim=9),
    # the longest horizon, one-layer encoder, 2 groups
    "t64": dict(dim=16, dim_mults=(1, 2, 4), horizon_steps=64, n_groups=2, smaller_encoder=True, diffusion_step_embed_dim=8,
                action_dim=2, cond_dim=6),
    # cond_dim near its limit at the narrowest padded width: the encoders' packed weight gradient (2 * 64 x 1016) is larger than
    # any conv's (the trainer's weight-gradient scratch is sized from the widest of the two)
    "cond_1000": dict(dim=64, dim_mults=(1,), horizon_steps=2, action_dim=2, cond_dim=1000),
}
NAMES = sorted(EDGE_SPECS)
CHAIN_NAMES = ["tiny_cg1", "l1_t1", "l4_default", "dec_40", "flat_64", "t64"]
PPO_NAMES = ["l4_default", "dec_40", "l1_t1"]
DDPM = dict(denoising_steps=20, ft_denoising_steps=10, randn_clip_value=3)
DDIM = dict(denoising_steps=100, ft_denoising_steps=5, use_ddim=True, ddim_steps=5, randn_clip_value=3,
            min_sampling_denoising_std=0.04)
CHAIN_CASES = [(n, "ddpm") for n in CHAIN_NAMES] + [("l4_default", "ddim")]
PPO_KW = dict(denoising_steps=20, ft_denoising_steps=10, clip_ploss_coef=0.01, clip_ploss_coef_base=0.001)
SEED_FWD, SEED_BASE, SEED_FT, SEED_MSE, SEED_CRITIC = 81, 21, 22, 51, 33


def spec(name):
    return O.UnetSpec(**EDGE_SPECS[name])


def n_params(name):
    return sum(int(np.prod(s)) for _, s, _ in O.unet_param_shapes(spec(name)))


B130_NAMES = sorted(NAMES, key=n_params)[:4]  # the ragged 130-row batch (two GEMM row tiles) only where it is cheap


def params(u, seed, dtype):
    return {k: v.to(dtype) for k, v in O.unet_init_params(u, seed).items()}


# ------------------------------------------------------------------ the oracle's side: float32 inputs, evaluated in `dtype`
# tiny_cg1 normalises groups of TWO values in every GroupNorm: xhat = +-d / sqrt(d^2 + eps) has slope 1 / sqrt(eps) = 316 where
# the two nearly coincide, and among 130 random rows some always do (the float32 ORACLE then misses the float64 one by
# 2e-5 .. 1e-4, seeds 1130 .. 1135).  Its batches are therefore the best-conditioned quarter of a pool four times as large,
# judged by the oracle alone (float32 against float64, row by row).
POOLED = {"tiny_cg1"}


def draw_fwd(u, B, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, u.horizon_steps, u.action_dim, generator=gen)
    t = torch.randint(0, 20, (B,), generator=gen)
    s = torch.rand(B, 1, u.cond_dim, generator=gen) * 2 - 1
    return x, t, s


def oracle_forward(u, dtype, x, t, s):
    # (rows are independent, and torch's group_norm refuses a lone row whose groups hold one value each -- tiny_cg1's second
    # level at B = 1 -- so the oracle always sees the batch twice over)
    B = x.shape[0]
    with torch.no_grad():
        return O.unet_forward(params(u, SEED_FWD, dtype), u, x.repeat(2, 1, 1).to(dtype), t.repeat(2),
                              s.repeat(2, 1, 1).to(dtype))[:B]


@functools.lru_cache(maxsize=None)
def fwd_inputs(name, B):
    u = spec(name)
    if name not in POOLED:
        return draw_fwd(u, B, 1000 + B)
    x, t, s = draw_fwd(u, 4 * B, 1000 + B)
    err = (oracle_forward(u, torch.float32, x, t, s).double() - oracle_forward(u, torch.float64, x, t, s)).abs().amax(dim=(1, 2))
    keep = torch.sort(torch.argsort(err)[:B]).values
    return x[keep], t[keep], s[keep]


@functools.lru_cache(maxsize=None)
def ref_forward(name, B, dtype=torch.float64):
    return oracle_forward(spec(name), dtype, *fwd_inputs(name, B)).numpy()


def chain_inputs(u, kw, B=3):
    gen = torch.Generator().manual_seed(7)
    n_steps = kw["ddim_steps"] if kw.get("use_ddim") else kw["denoising_steps"]
    state = torch.rand(B, 1, u.cond_dim, generator=gen) * 2 - 1
    noise = torch.randn(n_steps + 1, B, u.horizon_steps, u.action_dim, generator=gen)
    return state, noise


@functools.lru_cache(maxsize=None)
def ref_chain(name, mode, dtype=torch.float64):
    """(chains, trajectories, log-probs of the float64 oracle's own chains rounded to float32), all numpy"""
    u = spec(name)
    kw = DDIM if mode == "ddim" else DDPM
    cfg = make_cfg(u, kw)
    state, noise = chain_inputs(u, kw)
    base, ft = params(u, SEED_BASE, dtype), params(u, SEED_FT, dtype)
    traj, chains = O.sample_chain(cfg, u, base, ft, state.to(dtype), noise.to(dtype))
    scored = chains if dtype == torch.float64 else torch.from_numpy(ref_chain(name, mode)[0]).float()
    scored = scored.float()  # what the HIP path is handed
    with torch.no_grad():
        lp = O.chain_logprob(cfg, u, base, ft, state.to(dtype), scored.to(dtype))
    return chains.numpy(), traj.numpy(), lp.numpy()


# flat_64 normalises groups of 2 channels x 2 steps: with most seeds some group's variance comes close to eps and the float32
# ORACLE's gradient already differs from the float64 one by 5e-4 .. 3e-3 (seed 3: 2.3e-3 in down_modules.1.1's first conv).
# Seed 8 is the best conditioned of 3 .. 8 (1.4e-4); the CPU test below holds every row to a tenth of the bounds.
# l4_t16_k3 is the ReLU row: a gradient jumps where a ReLU input changes sign, and seed 3 puts one input of up_modules.0.1 at
# 1.7e-8 (the fp32 kernel, right to 1e-6, lands on the other side: 8e-3 in that block's conv bias).  Seed 42 keeps all 122,112
# ReLU inputs of the float64 oracle 2.1e-5 away from zero, the widest margin of seeds 3 .. 79 (a CPU test below holds 1e-5).
MSE_INPUT_SEED = {"flat_64": 8, "l4_t16_k3": 42}


def mse_inputs(u, N=12, K=20, seed=3):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, u.horizon_steps, u.action_dim, generator=gen) * 2 - 1
    state = torch.rand(N, 1, u.cond_dim, generator=gen) * 2 - 1
    t = torch.randint(0, K, (N,), generator=gen)
    noise = torch.randn(N, u.horizon_steps, u.action_dim, generator=gen)
    return x0, state, t, noise


@functools.lru_cache(maxsize=None)
def ref_mse(name, dtype=torch.float64):
    """(loss, {"g_<name>": gradient}) of the supervised loss, K = 20"""
    u = spec(name)
    x0, state, t, noise = mse_inputs(u, seed=MSE_INPUT_SEED.get(name, 3))
    prm = {k: v.requires_grad_(True) for k, v in params(u, SEED_MSE, dtype).items()}
    loss = O.denoise_mse_loss(20, u, prm, x0.to(dtype), state.to(dtype), t, noise.to(dtype))
    loss.backward()
    return float(loss.detach()), {f"g_{k}": (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in prm.items()}


@functools.lru_cache(maxsize=None)
def ppo_batch(name, N=16):
    """A gathered PPO minibatch built from the float64 oracle's own chain (ratios near 1), as float32 tensors"""
    u = spec(name)
    cfg = make_cfg(u, dict(PPO_KW, gamma_denoising=0.99, randn_clip_value=3))
    gen = torch.Generator().manual_seed(11)
    Kft, f64 = cfg.ft_denoising_steps, torch.float64
    state = torch.rand(N, 1, u.cond_dim, generator=gen) * 2 - 1
    noise = torch.randn(cfg.denoising_steps + 1, N, u.horizon_steps, u.action_dim, generator=gen)
    base, ft = params(u, 31, f64), params(u, 32, f64)
    _, chains = O.sample_chain(cfg, u, base, ft, state.to(f64), noise.to(f64))
    chains = chains.float()
    kinds = torch.randint(0, Kft, (N,), generator=gen)
    rows = torch.arange(N)
    with torch.no_grad():
        lp = O.chain_logprob(cfg, u, base, ft, state.to(f64), chains.to(f64)).reshape(N, Kft, u.horizon_steps, u.action_dim)
        val = O.critic_forward({k: v.to(f64) for k, v in O.init_params(CRITIC(u), SEED_CRITIC).items()}, CRITIC(u),
                               state.to(f64)).view(-1)
    oldlp = (lp[rows, kinds] + 0.02 * torch.randn(N, u.horizon_steps, u.action_dim, generator=gen)).float()
    oldv = (val + 0.3 * torch.randn(N, generator=gen)).float()
    ret = torch.randn(N, generator=gen)
    adv = 0.3 + 2.0 * torch.randn(N, generator=gen)
    return dict(state=state, prev=chains[rows, kinds].contiguous(), next=chains[rows, kinds + 1].contiguous(), kinds=kinds,
                returns=ret, oldvalues=oldv, adv=adv, oldlogprobs=oldlp, reward_horizon=min(4, u.horizon_steps))


@functools.lru_cache(maxsize=None)
def ref_ppo(name, dtype=torch.float64):
    """(the 8 statistics, {"gactor_<name>" / "gcritic_<name>": gradient}) of pg_loss + 0.5 v_loss"""
    u = spec(name)
    c = CRITIC(u)
    cfg = make_cfg(u, dict(PPO_KW, gamma_denoising=0.99, randn_clip_value=3))
    b = ppo_batch(name)
    ft = {k: v.requires_grad_(True) for k, v in params(u, 32, dtype).items()}
    cr = {k: v.to(dtype).requires_grad_(True) for k, v in O.init_params(c, SEED_CRITIC).items()}
    f = lambda k: b[k].to(dtype)
    res = O.ppo_loss(cfg, u, c, params(u, 31, dtype), ft, cr, f("state"), f("prev"), f("next"), b["kinds"], f("returns"),
                     f("oldvalues"), f("adv"), f("oldlogprobs"), reward_horizon=b["reward_horizon"])
    stats = np.array([res[0].item(), float(res[1]), res[2].item(), res[3], res[4], res[5], float(res[6]), res[7]])
    (res[0] + 0.5 * res[2]).backward()
    g = {f"gactor_{k}": (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in ft.items()}
    g.update({f"gcritic_{k}": v.grad.numpy() for k, v in cr.items()})
    return stats, g


# ------------------------------------------------------------------ what bf16 operands alone cost: the oracle, rounded
class _RoundedF:
    """torch.nn.functional with the weights and the input of every convolution / linear layer rounded through bfloat16
    (straight-through for autograd); accumulation, biases and everything between the GEMMs stay in the caller's precision"""

    def __getattr__(self, k):
        return getattr(torch.nn.functional, k)

    @staticmethod
    def _r(x):
        return x + (x.to(torch.bfloat16).to(x.dtype) - x).detach()

    def conv1d(self, x, w, b=None, **kw):
        return torch.nn.functional.conv1d(self._r(x), self._r(w), b, **kw)

    def conv_transpose1d(self, x, w, b=None, **kw):
        return torch.nn.functional.conv_transpose1d(self._r(x), self._r(w), b, **kw)

    def linear(self, x, w, b=None):
        return torch.nn.functional.linear(self._r(x), self._r(w), b)


@contextlib.contextmanager
def bf16_operands():
    real, O.F = O.F, _RoundedF()
    try:
        yield
    finally:
        O.F = real


# Rows whose bf16 bounds come from the rounded oracle instead of tests/test_unet.py: flat_64 normalises groups of 4 values, and
# bf16 OPERANDS alone (float64 arithmetic, no kernel) move its chain by 0.124 and turn its gradient to cosine 0.825 against the
# unrounded oracle.  The bound is twice that distance; every fp32 bound, and bf16 elsewhere, stays.
BF16_FROM_ROUNDED_ORACLE = {"flat_64"}


@functools.lru_cache(maxsize=None)
def bf16_chain_distance(name, mode):
    """max |chains|, max |trajectories| between the float64 oracle with bf16 operands and the float64 oracle"""
    u = spec(name)
    kw = DDIM if mode == "ddim" else DDPM
    state, noise = chain_inputs(u, kw)
    f64 = torch.float64
    with bf16_operands():
        traj, chains = O.sample_chain(make_cfg(u, kw), u, params(u, SEED_BASE, f64), params(u, SEED_FT, f64), state.to(f64),
                                      noise.to(f64))
    c0, t0, _ = ref_chain(name, mode)
    return float(np.abs(chains.numpy() - c0).max()), float(np.abs(traj.numpy() - t0).max())


@functools.lru_cache(maxsize=None)
def bf16_mse_cosine(name):
    """cosine of the whole gradient of the float64 oracle with bf16 operands against the float64 oracle's"""
    u = spec(name)
    f64 = torch.float64
    x0, state, t, noise = mse_inputs(u, seed=MSE_INPUT_SEED.get(name, 3))
    prm = {k: v.requires_grad_(True) for k, v in params(u, SEED_MSE, f64).items()}
    with bf16_operands():
        O.denoise_mse_loss(20, u, prm, x0.to(f64), state.to(f64), t, noise.to(f64)).backward()
    g = ref_mse(name)[1]
    x = np.concatenate([g[f"g_{k}"].reshape(-1) for k in prm])
    y = np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(-1) for v in prm.values()])
    return float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y)))


def named(g, prefix):
    return [(k[len(prefix) + 1:], torch.from_numpy(v)) for k, v in g.items() if k.startswith(prefix + "_")]


# ------------------------------------------------------------------ CPU: the reference itself, and the parameter order
@pytest.mark.parametrize("name", NAMES)
def test_oracle_float32_agrees_with_float64_to_a_tenth_of_every_bound(name):
    """The fp32 bounds of the GPU tests below are for the KERNEL's error: the reference's own rounding (the oracle in float32,
    as the fixtures of tests/test_unet.py hold it, against the oracle in float64) must stay under a tenth of each.  A row that
    comes closer is badly conditioned input (change the seed, never the bound)."""
    f32 = torch.float32
    for B in (1, 5) + ((130,) if name in B130_NAMES else ()):
        np.testing.assert_allclose(ref_forward(name, B, f32), ref_forward(name, B), rtol=2e-5, atol=2e-5)
    for n, mode in CHAIN_CASES:
        if n != name:
            continue
        (c32, t32, l32), (c64, t64, l64) = ref_chain(name, mode, f32), ref_chain(name, mode)
        np.testing.assert_allclose(c32, c64, rtol=5e-5, atol=5e-5)
        np.testing.assert_allclose(t32, t64, rtol=5e-5, atol=5e-5)
        sel = l64 > -50
        np.testing.assert_allclose(l32[sel], l64[sel], rtol=2e-4, atol=2e-4)
        assert np.abs(l32[sel] - l64[sel]).mean() <= 2e-5
    (loss32, g32), (loss64, g64) = ref_mse(name, f32), ref_mse(name)
    assert loss32 == pytest.approx(loss64, rel=2e-5)
    worst, norm = grad_report(g64, "g", named(g32, "g"))
    assert worst[1] <= 5e-4 and norm <= 2e-4, (worst, norm)
    if name in PPO_NAMES:
        (s32, g32), (s64, g64) = ref_ppo(name, f32), ref_ppo(name)
        np.testing.assert_allclose(s32, s64, rtol=5e-5, atol=5e-6)
        worst, norm = grad_report(g64, "gactor", named(g32, "gactor"))
        assert worst[1] <= 5e-4 and norm <= 2e-4, (worst, norm)
        worst, norm = grad_report(g64, "gcritic", named(g32, "gcritic"))
        assert worst[1] <= 2e-4 and norm <= 1e-4, (worst, norm)


@pytest.mark.parametrize("name", [n for n in NAMES if EDGE_SPECS[n].get("activation") == "ReLU"])
def test_relu_rows_keep_clear_of_the_kink(name, monkeypatch):
    """A ReLU input within the fp32 kernel's rounding of zero (about 1e-6 after a GroupNorm) makes the gradient check a coin
    toss that no kernel can win: the supervised-loss inputs of a ReLU row keep every ReLU input 1e-5 away from it."""
    u = spec(name)
    seen = []
    monkeypatch.setitem(O._ACT, "ReLU", lambda x: (seen.append(float(x.detach().abs().min())), torch.relu(x))[1])
    f64 = torch.float64
    x0, state, t, noise = mse_inputs(u, seed=MSE_INPUT_SEED.get(name, 3))
    with torch.no_grad():
        O.denoise_mse_loss(20, u, params(u, SEED_MSE, f64), x0.to(f64), state.to(f64), t, noise.to(f64))
    assert len(seen) > 0 and min(seen) >= 1e-5, min(seen)


@pytest.mark.parametrize("name", sorted(BF16_FROM_ROUNDED_ORACLE))
def test_bf16_bounds_from_the_rounded_oracle_are_needed_and_recorded(name):
    """The rows that take a bf16 bound from the rounded oracle are those where bf16 operands alone pass the usual one (else the
    usual bound stands), and the distances are the ones DESIGN.md records."""
    chain, traj = bf16_chain_distance(name, "ddpm")
    cos = bf16_mse_cosine(name)
    assert chain > 8e-2 / 2 and 1.0 - cos > (1.0 - 0.98) / 2, (chain, cos)
    if name == "flat_64":
        assert chain == pytest.approx(0.124, abs=2e-3) and cos == pytest.approx(0.825, abs=2e-3), (chain, traj, cos)


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_names_and_order_match_the_reference(name):
    u = spec(name)
    m = hip_unet(u, 1, "fp32", dev="cpu")
    want = [n for n, _, _ in O.unet_param_shapes(u)]
    assert [k for k, _ in m.named_parameters()] == want
    assert list(m.state_dict()) == want
    assert [tuple(p.shape) for p in m.parameters()] == [s for _, s, _ in O.unet_param_shapes(u)]


# ------------------------------------------------------------------ GPU
DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("bf16", 6e-2)])
@pytest.mark.parametrize("name", NAMES)
def test_hip_forward(name, prec, tol):
    """Unet1D.forward (dppo_unet_forward) at B = 1, 5 (and 130 for the four smallest networks)."""
    u = spec(name)
    m = hip_unet(u, SEED_FWD, prec)
    for B in (1, 5) + ((130,) if name in B130_NAMES else ()):
        x, t, s = fwd_inputs(name, B)
        got = m(x.to(DEV), t.to(DEV), {"state": s.to(DEV)}).cpu().numpy()
        want = ref_forward(name, B)
        print(f"{name} {prec} B={B}: max |err| {np.abs(got - want).max():.3e} (|ref| max {np.abs(want).max():.3f})")
        np.testing.assert_allclose(got, want, rtol=tol, atol=tol, err_msg=f"B={B}")


def ppo_model(u, prec, kw, seeds=(SEED_BASE, SEED_FT), critic_seed=None, **extra):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.diffusion_ppo import PPODiffusion
    from dppo_amd.model.diffusion.eta import EtaFixed
    actor = hip_unet(u, seeds[0], prec, dev="cpu")
    critic = CriticObs(cond_dim=u.cond_dim, mlp_dims=[256, 256, 256], residual_style=True, precision=prec)
    if critic_seed is not None:
        critic.load_state_dict(O.init_params(CRITIC(u), critic_seed))
    kw2 = dict(kw, eta=EtaFixed(base_eta=1.0)) if kw.get("use_ddim") else dict(kw)
    m = PPODiffusion(actor=actor, critic=critic, horizon_steps=u.horizon_steps, obs_dim=u.cond_dim, action_dim=u.action_dim,
                     device=DEV, gamma_denoising=0.99, **dict(kw2, **extra))
    m.actor_ft.load_state_dict(O.unet_init_params(u, seeds[1]), strict=True)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,mode", CHAIN_CASES)
def test_hip_chains_and_logprobs(name, mode, prec):
    """The sampler (FiLM tables precomputed for all steps) and the log-prob evaluation (unet_chain_input_kernel /
    unet_cond_rows_kernel), with recorded noise, against O.sample_chain / O.chain_logprob."""
    u = spec(name)
    kw = DDIM if mode == "ddim" else DDPM
    m = ppo_model(u, prec, kw, clip_ploss_coef=0.01)
    state, noise = chain_inputs(u, kw)
    chains, traj, ref = ref_chain(name, mode)
    smp = m(cond={"state": state.to(DEV)}, deterministic=False, return_chain=True, noise=noise.to(DEV))
    assert tuple(smp.chains.shape) == chains.shape
    ct = tt = 5e-4 if prec == "fp32" else 8e-2
    if prec == "bf16" and name in BF16_FROM_ROUNDED_ORACLE:
        ct, tt = (2 * v for v in bf16_chain_distance(name, mode))
    print(f"{name} {mode} {prec}: chains max |err| {np.abs(smp.chains.cpu().numpy() - chains).max():.3e} (bound {ct:.3e})")
    np.testing.assert_allclose(smp.chains.cpu().numpy(), chains, rtol=ct, atol=ct)
    np.testing.assert_allclose(smp.trajectories.cpu().numpy(), traj, rtol=tt, atol=tt)
    lp = m.get_logprobs({"state": state.to(DEV)}, torch.from_numpy(chains).float().to(DEV)).cpu().numpy()
    sel = ref > -50
    assert sel.any()
    lt = 2e-3 if prec == "fp32" else 1.0
    print(f"{name} {mode} {prec}: logp max |err| {np.abs(lp[sel] - ref[sel]).max():.3e} mean {np.abs(lp[sel] - ref[sel]).mean():.3e}")
    np.testing.assert_allclose(lp[sel], ref[sel], rtol=lt, atol=lt)
    assert np.abs(lp[sel] - ref[sel]).mean() <= (2e-4 if prec == "fp32" else 0.15)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_denoise_mse_and_grads(name):
    """DiffusionModel.p_losses (forward with a tape + the mirrored backward): the loss and EVERY parameter gradient."""
    from dppo_amd.model.diffusion.diffusion import DiffusionModel
    u = spec(name)
    x0, state, t, noise = (v.to(DEV) for v in mse_inputs(u, seed=MSE_INPUT_SEED.get(name, 3)))
    want, g = ref_mse(name)
    flat = {}
    for prec in ("fp32", "bf16"):
        net = hip_unet(u, SEED_MSE, prec, dev="cpu")
        m = DiffusionModel(network=net, horizon_steps=u.horizon_steps, obs_dim=u.cond_dim, action_dim=u.action_dim, device=DEV,
                           denoising_steps=20)
        loss = m.p_losses(x0, {"state": state}, t, noise=noise)
        loss.backward()
        flat[prec] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).double().cpu().numpy()
        print(f"{name} {prec}: loss {loss.item():.6f} ref {want:.6f}")
        if prec == "fp32":
            worst, norm = grad_report(g, "g", [(k, p.grad) for k, p in net.named_parameters()])
            print(f"{name} fp32: worst tensor {worst}, norm ratio - 1 {norm:.3e}")
            assert loss.item() == pytest.approx(want, rel=2e-4)
            assert worst[1] <= 5e-3 and norm <= 2e-3, (worst, norm)
        else:
            assert loss.item() == pytest.approx(want, rel=3e-2)
    x, y = flat["fp32"], flat["bf16"]
    cos = float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y)))
    floor = 0.98 if name not in BF16_FROM_ROUNDED_ORACLE else 1.0 - 2 * (1.0 - bf16_mse_cosine(name))
    print(f"{name}: cos(fp32, bf16) {cos:.5f} (floor {floor:.5f})")
    assert cos >= floor


@pytest.mark.gpu
@pytest.mark.parametrize("name", PPO_NAMES)
def test_hip_ppo_loss_and_grads(name):
    """PPODiffusion.loss, gathered mode (dppo_unet_ppo_loss_fwd_bwd), fp32: the statistics, every actor and critic gradient."""
    u = spec(name)
    b = ppo_batch(name)
    stats, g = ref_ppo(name)
    m = ppo_model(u, "fp32", PPO_KW, seeds=(31, 32), critic_seed=SEED_CRITIC, randn_clip_value=3)
    d = lambda k: b[k].to(DEV)
    res = m.loss({"state": d("state")}, d("prev"), d("next"), d("kinds"), d("returns"), d("oldvalues"), d("adv"),
                 d("oldlogprobs"), use_bc_loss=False, reward_horizon=b["reward_horizon"])
    got = np.array([res[0].item(), float(res[1]), res[2].item(), res[3], res[4], res[5], float(res[6]), res[7]])
    print(f"{name}: stats {got} ref {stats}")
    np.testing.assert_allclose(got, stats, rtol=5e-4, atol=5e-5)
    (res[0] + 0.5 * res[2]).backward()
    worst, norm = grad_report(g, "gactor", [(k, p.grad) for k, p in m.actor_ft.named_parameters()])
    print(f"{name}: actor worst {worst} norm {norm:.3e}")
    assert worst[1] <= 5e-3 and norm <= 2e-3, (worst, norm)
    worst, norm = grad_report(g, "gcritic", [(k, p.grad) for k, p in m.critic.named_parameters()])
    assert worst[1] <= 2e-3 and norm <= 1e-3, (worst, norm)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PPO_NAMES)
def test_hip_update_in_rollout_mode(name):
    """ppo_update straight from a rollout buffer, fp32 and bf16: ratio == 1 against the model's own log-probs (the inference
    and the training forward are two kernel chains over the same images), finite gradients, the critic's direction kept."""
    from dppo_amd import hip
    u = spec(name)
    out = {}
    for prec in ("fp32", "bf16"):
        m = ppo_model(u, prec, DDPM, seeds=(41, 42), critic_seed=43, clip_ploss_coef=0.01)
        R, Kft, AF, N = 24, 10, u.horizon_steps * u.action_dim, 100
        gen = torch.Generator().manual_seed(2)
        obs = (torch.rand(R, 1, u.cond_dim, generator=gen) * 2 - 1).to(DEV)
        noise = torch.randn(21, R, AF, generator=gen).to(DEV)
        chains = m(cond={"state": obs}, noise=noise).chains
        logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF)
        val = m.critic({"state": obs}).reshape(R)
        ret, adv = val + torch.randn(R, generator=gen).to(DEV), torch.randn(R, generator=gen).to(DEV)
        inds = torch.randperm(R * Kft, generator=gen)[:N].to(DEV).contiguous()
        st = m.ppo_update(obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), ret, val, adv, logp,
                          inds).cpu().numpy().copy()
        print(f"{name} {prec}: ratio - 1 = {st[hip.STAT_RATIO] - 1.0:.3e}")
        assert st[hip.STAT_RATIO] == pytest.approx(1.0, abs=1e-5 if prec == "fp32" else 1e-3)
        ga = m.actor_ft.flat_grads().double().cpu().numpy().copy()
        gc = m.critic.flat_grads().double().cpu().numpy().copy()
        assert np.isfinite(ga).all() and np.isfinite(gc).all() and np.linalg.norm(ga) > 0
        out[prec] = (ga, gc)
    cos = lambda x, y: float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y) + 1e-30))
    assert cos(out["fp32"][1], out["bf16"][1]) >= 0.99
