"""The residual MLP trunks (DiffusionMLP actor, CriticObs critic: csrc/api.hip, fused.hip, sampler.hip) over the descriptor
space check_net() accepts, not just the named networks of tests/test_hip_parity.py: hidden widths off the fused kernels' three
(128, 384, 768, 1152: the layered GEMM chain), zero / two / eight blocks, out_dim 1 .. 128 around the merged forward's limits
(16 | 17, 64 | 65), in_dim above hidden and at 1024, time_dim 4 .. 36, encoder widths on both sides of a multiple of 16, and the
column budgets of the in-kernel first-layer gradient.  The HIP path runs against the oracle (oracle/dppo_oracle.py) evaluated in
float64 on the CPU inside the test (no fixtures).  CPU tests keep the comparison honest: every route the GPU tests take is
pinned in a literal table that shows every route bit set and clear; the oracle in float32 agrees with the oracle in float64 to a
tenth of every fp32 bound; every non-smooth decision of the float64 oracle keeps a guard band on the chosen inputs; the flat
parameter layout; one refusal per line of check_net().  fp32 bounds are those of tests/test_hip_parity.py, bf16 bounds those of
tests/test_hip_parity.py and tests/test_bf16_parity.py, or twice what bf16 operands alone cost the float64 oracle where that
is more than half of one (BF16_FROM_ROUNDED_ORACLE).

Measured on an MI355X, as the worst check in units of its bound (DESIGN.md 4.2 has every row): fp32 forward at most 0.060 of 2e-5
(h256_ln_nb8, B = 130), fp32 chains / log-probs 0.011 (h512_out128), fp32 gradient tensors 0.026 (h256_ln_nb8, M = 80), the
float32 oracle itself under a tenth of each; bf16 forward 0.37 (h256_ln_nb8), chains 0.39 (h512_out128), denoising-loss gradients
0.55 (h128_out1), PPO 0.82 (h512_ln_nb2, time_embedding.1.bias norm at M = 80), BC term 0.19.  On the checks whose bound is twice
the bf16-operand yardstick the kernels' worst distance, in yardsticks (2 is the bound): h128_out1 1.10, h1152 1.00, h256_nb0
0.75, h768 0.65, h384_nb2 0.63, h256_room 0.61, h256_ln_nb8 0.40, h512_ln_nb2 0.39, h512_out65 0.25, h256_af3 0.14, h256_round
0.07, h512_out64 0.07.  No row showed a wrong number, a fault or a mis-route; no kernel changed.

Refused by name (the sampler kernel does not launch): the K-step sampler at hidden 128, 384, 1152 ("not instantiated") and, in fp32, at
in_dim 1024 / hidden 1024 ("LDS image exceeds 160 KiB": 16 rows x (1024 + 2 x 1024) floats)."""
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import dppo_oracle as O
from tests.test_oracle_golden import make_cfg
from tests.test_route import BITS, PPO_ACTOR, PPO_CRITIC, SIDE, route
from tests.test_vision_specs import _RoundedF, cos_ratio, oracle_functional

T = torch.from_numpy
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


def _a(Ta, Da, cond, td, dims, act, ln=False, enc=None):
    return dict(kind="actor", horizon_steps=Ta, action_dim=Da, cond_dim=cond, time_dim=td, mlp_dims=list(dims), activation=act,
                residual=True, use_layernorm=ln, cond_mlp_dims=enc)


def _c(cond, dims, act, ln=False):
    return dict(kind="critic", cond_dim=cond, mlp_dims=list(dims), activation=act, residual=True, use_layernorm=ln)


EDGE_ACTORS = {
    "h128_out1": _a(1, 1, 1, 4, [128] * 3, "Mish"),            # smallest accepted everything; layered; the sampler refuses
    "h384_nb2": _a(2, 3, 5, 6, [384] * 5, "ReLU"),             # layered, two blocks, time_dim % 4 != 0
    "h768": _a(4, 7, 9, 32, [768] * 3, "Mish"),                # sampler TPW 6 / OT 4; the loss is layered
    "h1152": _a(4, 3, 11, 16, [1152] * 3, "Mish"),             # above 1024: layered; the sampler refuses
    "h256_nb0": _a(4, 3, 11, 16, [256], "ReLU"),               # no block at all: never low-rank, no activation anywhere
    "h256_nb2": _a(4, 3, 11, 16, [256] * 5, "Mish"),           # general fused backward with a low-rank top
    "h256_ln_nb8": _a(3, 2, 7, 8, [256] * 17, "Mish", ln=True),    # MAX_BLOCKS, with LayerNorm
    "h512_ln_nb2": _a(4, 3, 11, 16, [512] * 5, "ReLU", ln=True),   # LayerNorm + ReLU at 512, two blocks
    "h512_out16": _a(4, 4, 8, 8, [512] * 3, "ReLU"),           # fused_can_merge: the last narrow head (bf16 merges, fp32 does not)
    "h512_out17": _a(1, 17, 8, 8, [512] * 3, "ReLU"),          # fused_can_merge: the first wide head
    "h512_out64": _a(8, 8, 8, 8, [512] * 3, "Mish"),           # fused_can_merge: the last wide head (bf16 only)
    "h512_out65": _a(5, 13, 8, 8, [512] * 3, "Mish"),          # fused_can_merge: one past it, merges in neither precision
    "h512_out128": _a(16, 8, 8, 8, [512] * 3, "Mish"),         # the widest head, OT 8; lowrank_top needs M >= 12800
    "h256_room": _a(2, 2, 8, 16, [256] * 3, "ReLU"),           # dW0: 4 + 8 columns, room 20 >= Kft 10: every one-hot, no rounding
    "h256_round": _a(2, 2, 19, 16, [256] * 3, "ReLU"),         # room 9 = Kft - 1: dW0 with dw0_round
    "h256_noroom": _a(2, 2, 20, 16, [256] * 3, "ReLU"),        # room 8 < Kft - 1: dW0 off
    "h256_af3": _a(1, 3, 8, 16, [256] * 3, "ReLU"),            # act_flat % 4 != 0: no dW0, the one-hot columns stay
    "h256_td36": _a(2, 2, 8, 36, [256] * 3, "ReLU"),           # 32 + time_dim > 64: no dW0, the one-hot columns stay
    "h256_enc8": _a(2, 2, 20, 16, [256] * 3, "Mish", enc=[24, 8]),    # cond_out % 16 != 0: no one-hot columns
    "h256_enc16": _a(2, 2, 20, 16, [256] * 3, "Mish", enc=[24, 16]),  # cond_out % 16 == 0: one-hot columns
    "h256_in320": _a(2, 2, 300, 16, [256] * 3, "ReLU"),        # Kp0 > hidden: not fused (layered), though one_block is reported
    "h1024_in1024": _a(2, 2, 1004, 16, [1024] * 3, "ReLU"),    # in_dim at its limit, Kp0 = hidden = 1024
    # the partners of three critic rows, whose observation width no actor row above has (a critic reads its actor's observation)
    "h256_c32": _a(2, 2, 32, 16, [256] * 3, "Mish"),           # act_flat + cond_dim = 36 > 32 columns: no dW0 (its critic takes it)
    "h256_c33": _a(2, 2, 33, 16, [256] * 3, "Mish"),           # the same, beside c256_in33
    "h256_enc_c1024": _a(2, 2, 1024, 16, [256] * 3, "Mish", enc=[32, 16]),  # an encoder over 1024 observation columns (Kpc = 1024)
}
EDGE_CRITICS = {
    "c128_nb0": _c(1, [128], "ReLU"),                          # the empty route: layered, no block, one input column
    "c256_in32": _c(32, [256] * 3, "Mish"),                    # in_dim <= 32: dW0 on the critic; N = 99 | 100 flips one_block, lowrank
    "c256_in33": _c(33, [256] * 3, "Mish"),                    # in_dim > 32: dW0 off
    "c512_ln_nb2": _c(11, [512] * 5, "Mish", ln=True),         # LayerNorm critic, two blocks
    "c768": _c(11, [768] * 3, "Mish"),                         # layered critic
    "c1024_in1024": _c(1024, [1024] * 3, "ReLU"),              # in_dim at its limit
}
ACTOR_NAMES, CRITIC_NAMES = sorted(EDGE_ACTORS), sorted(EDGE_CRITICS)
SAMPLER_WIDTHS = (256, 512, 768, 1024)
# (row, precision) -> the library's message where the K-step sampler refuses a row
SAMPLER_REFUSED = {(n, p): "not instantiated" for n in ACTOR_NAMES for p in ("fp32", "bf16")
                   if EDGE_ACTORS[n]["mlp_dims"][0] not in SAMPLER_WIDTHS}
SAMPLER_REFUSED[("h1024_in1024", "fp32")] = "LDS image exceeds 160 KiB"
SEED_FWD, SEED_BASE, SEED_MSE, SEED_CRITIC = 11, 21, 51, 33
K, KFT = 20, 10


def spec(name):
    if name.startswith("std"):  # the usual critic ([256, 256, 256], Mish) on std<cond_dim> observation columns: no row of the table,
        return O.NetSpec(**_c(int(name[3:]), [256] * 3, "Mish"))  # the partner of an actor whose cond_dim no critic row has
    return O.NetSpec(**(EDGE_ACTORS[name] if name in EDGE_ACTORS else EDGE_CRITICS[name]))


def hip_net(name, seed, prec, dev=DEV):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    s = spec(name)
    if s.kind == "actor":
        m = DiffusionMLP(action_dim=s.action_dim, horizon_steps=s.horizon_steps, cond_dim=s.cond_dim, time_dim=s.time_dim,
                         mlp_dims=list(s.mlp_dims), activation_type=s.activation, cond_mlp_dims=s.cond_mlp_dims, residual_style=True,
                         use_layernorm=s.use_layernorm, precision=prec)
    else:
        m = CriticObs(cond_dim=s.cond_dim, mlp_dims=list(s.mlp_dims), activation_type=s.activation, residual_style=True,
                      use_layernorm=s.use_layernorm, precision=prec)
    m.load_state_dict(O.init_params(s, seed), strict=True)
    return m.to(dev) if dev != "cpu" else m


@functools.lru_cache(maxsize=None)
def actor_desc(name):
    return hip_net(name, 1, "fp32", dev="cpu").net_desc()


def params(s, seed, dtype):
    return {k: v.to(dtype) for k, v in O.init_params(s, seed).items()}


def ft_params(s, dtype, mix=1.0):
    """the fine-tuned network: seed SEED_BASE + 1, or (mix < 1) the base network moved that fraction of the way towards it"""
    b, f = O.init_params(s, SEED_BASE), O.init_params(s, SEED_BASE + 1)
    return {k: (b[k] + np.float32(mix) * (f[k] - b[k])).to(dtype) for k in b}


# ------------------------------------------------------------------ the oracle in float64 / float32 / with bf16 operands
class _CastF:
    """torch.nn.functional whose linear() takes its input to the weight's dtype: the oracle's sinusoidal() is float32 by
    construction (as the reference's), everything behind it runs in the parameters' precision"""

    def __getattr__(self, k):
        return getattr(torch.nn.functional, k)

    def linear(self, x, w, b=None):
        return torch.nn.functional.linear(x.to(w.dtype), w, b)


class _RoundedCastF(_RoundedF):
    """tests/test_vision_specs.py's bf16-operand functional (weights, input and output gradient of every Linear rounded through
    bfloat16, accumulation and everything between the GEMMs in the caller's precision) behind the same cast"""

    def linear(self, x, w, b=None):
        assert w.shape[0] != 3 * w.shape[1]  # (what _RoundedF takes for a qkv projection; no trunk here has such a layer)
        return super().linear(x.to(w.dtype), w, b)


@contextlib.contextmanager
def oracle_mode(rounded=False, relu_log=None):
    """relu_log: a list that receives, per ReLU call, the per-row smallest |input| (a tensor over the rows)"""
    relu = O._ACT["ReLU"]
    if relu_log is not None:
        O._ACT["ReLU"] = lambda x: (relu_log.append(x.detach().abs().reshape(x.shape[0], -1).amin(dim=1)), relu(x))[1]
    try:
        with oracle_functional(_RoundedCastF() if rounded else _CastF()):
            yield
    finally:
        O._ACT["ReLU"] = relu


MODES = {"f64": (F64, False), "f32": (F32, False), "bf16ops": (F64, True)}  # oracle mode -> (dtype, bf16 operands)


# ------------------------------------------------------------------ forward
FWD_BATCHES = (1, 17, 130)  # one row, a ragged tile, two row tiles


def fwd_inputs(name, B):
    s = spec(name)
    gen = torch.Generator().manual_seed(1000 + B)
    st = torch.rand(B, 1, s.cond_dim, generator=gen) * 2 - 1
    if s.kind == "critic":
        return (st,)
    return torch.randn(B, s.horizon_steps, s.action_dim, generator=gen), torch.randint(0, K, (B,), generator=gen), st


@functools.lru_cache(maxsize=None)
def ref_forward(name, B, mode="f64"):
    s = spec(name)
    dtype, rounded = MODES[mode]
    p = params(s, SEED_FWD, dtype)
    with torch.no_grad(), oracle_mode(rounded):
        if s.kind == "critic":
            return O.critic_forward(p, s, fwd_inputs(name, B)[0].to(dtype)).numpy()
        x, t, st = fwd_inputs(name, B)
        return O.actor_forward(p, s, x.to(dtype), t, st.to(dtype)).numpy()


# ------------------------------------------------------------------ sampling chain and chain log-probs
DDPM = dict(denoising_steps=K, ft_denoising_steps=KFT, randn_clip_value=3, final_action_clip_value=1.0)
DDIM = dict(denoising_steps=100, ft_denoising_steps=5, use_ddim=True, ddim_steps=5, randn_clip_value=3, eps_clip_value=0.7,
            min_sampling_denoising_std=0.04)
CHAIN_KW = {"ddpm": DDPM, "ddim": DDIM}
CHAIN_BATCHES = (3, 17)
CHAIN_CASES = [(n, "ddpm") for n in ACTOR_NAMES] + [("h768", "ddim"), ("h512_out65", "ddim")]


def _chain_draw(s, n_steps, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 1, s.cond_dim, generator=gen) * 2 - 1,
            torch.randn(n_steps + 1, n, s.horizon_steps, s.action_dim, generator=gen))


def chain_bounds(kw):
    """the bounds of the sampler's per-entry clamps: x0 and the final action at 1, the eps clamp, the noise clamp"""
    return sorted({1.0, float(kw["randn_clip_value"])} | ({float(kw["eps_clip_value"])} if "eps_clip_value" in kw else set()))


@functools.lru_cache(maxsize=None)
def chain_inputs(name, mode, B):
    """(state, noise): the first B rows of a pool of B + B // 2 + 4 (B drawn, then the spares from a second seed) on which the
    float64 oracle, sampling and then scoring its own chain, keeps every entry of x0, of the final action, of eps and of the
    noise 1.5 CLAMP_BAND from the clamp's bound -- rows are independent, so the choice is judged by the oracle alone, row by row"""
    s, kw = spec(name), CHAIN_KW[mode]
    n_steps = kw["ddim_steps"] if kw.get("use_ddim") else kw["denoising_steps"]
    state, noise = (torch.cat(v, dim=d) for d, v in enumerate(zip(_chain_draw(s, n_steps, B, 7 + B),
                                                                    _chain_draw(s, n_steps, B // 2 + 4, 7007 + B))))
    cfg, base, ft = make_cfg(s, kw), params(s, SEED_BASE, F64), ft_params(s, F64)
    with oracle_mode(), _Decisions(rows=state.shape[0], bounds=chain_bounds(kw)) as d, torch.no_grad():
        chains = O.sample_chain(cfg, s, base, ft, state.double(), noise.double())[1]
        O.chain_logprob(cfg, s, base, ft, state.double(), chains.float().double())
    keep = torch.nonzero(torch.stack(d.per_row).amin(dim=0) >= 1.5 * CLAMP_BAND).reshape(-1)
    assert len(keep) >= B, (name, mode, B, len(keep))
    return state[keep[:B]], noise[:, keep[:B]].contiguous()


@functools.lru_cache(maxsize=None)
def ref_chain(name, mode, B, omode="f64"):
    """(chains, trajectories, log-probs of the FLOAT64 oracle's own chains as the HIP path is handed them), numpy"""
    s, kw = spec(name), CHAIN_KW[mode]
    dtype, rounded = MODES[omode]
    cfg = make_cfg(s, kw)
    state, noise = chain_inputs(name, mode, B)
    base, ft = params(s, SEED_BASE, dtype), ft_params(s, dtype)
    with oracle_mode(rounded):
        traj, chains = O.sample_chain(cfg, s, base, ft, state.to(dtype), noise.to(dtype))
        scored = chains.float() if omode == "f64" else T(ref_chain(name, mode, B)[0]).float()
        with torch.no_grad():
            lp = O.chain_logprob(cfg, s, base, ft, state.to(dtype), scored.to(dtype))
    return chains.numpy(), traj.numpy(), lp.numpy()


class _Decisions:
    """Every clamp / clip the oracle takes between entering and leaving: (bound, smallest |x - bound|) per call and side.
    rows, bounds: also, per call and side of a clamp of a (rows, ...) tensor at +-one of the bounds, that distance row by row
    (a chain log-prob pass folds its Kft steps into the rows: (rows * Kft, ...), row-major)."""

    def __init__(self, rows=None, bounds=()):
        self.seen, self.per_row, self.rows, self.bounds = [], [], rows, tuple(bounds)

    def note(self, x, lo, hi):
        for b in (lo, hi):
            if b is not None and x.numel():
                bt = b.detach().to(x.dtype) if torch.is_tensor(b) else torch.tensor(float(b), dtype=x.dtype)
                dist = (x.detach() - bt).abs()
                self.seen.append((float(bt.reshape(-1)[0]), float(dist.min())))
                if self.rows and not torch.is_tensor(b) and abs(float(b)) in self.bounds:
                    assert x.shape[0] % self.rows == 0
                    self.per_row.append(dist.reshape(self.rows, -1).amin(dim=1))

    def __enter__(self):
        self.real = (torch.Tensor.clamp, torch.clamp, torch.clip)
        meth, fn, clip = self.real

        def args(a, kw):
            lo = a[0] if len(a) > 0 else kw.get("min")
            hi = a[1] if len(a) > 1 else kw.get("max")
            return lo, hi

        def w_meth(x, *a, **kw):
            self.note(x, *args(a, kw))
            return meth(x, *a, **kw)

        def w_fn(x, *a, **kw):
            self.note(x, *args(a, kw))
            return fn(x, *a, **kw)

        def w_clip(x, *a, **kw):
            self.note(x, *args(a, kw))
            return clip(x, *a, **kw)
        torch.Tensor.clamp, torch.clamp, torch.clip = w_meth, w_fn, w_clip
        return self

    def __exit__(self, *exc):
        torch.Tensor.clamp, torch.clamp, torch.clip = self.real

    def nearest(self, bound):
        return min((d for b, d in self.seen if abs(abs(b) - bound) < 1e-6 * bound), default=None)  # (a float32 table's 0.1 is 0.1 + 1.5e-9)


# ------------------------------------------------------------------ the supervised (denoising-MSE) loss
MSE_BATCHES = (12, 130)
RELU_BAND = 1e-5   # every ReLU input of the float64 oracle stays this far from zero (tests/test_unet_specs.py's band)
CLAMP_BAND = 1e-5  # ... and every clamped quantity (x0, the final action, eps, the noise, the step's std, log-probs at -5 / 2) from its bound
RATIO_BAND = 5e-3  # |ratio - 1| against the clip range: wide enough for bf16 too (test_bf16_parity holds the ratio to 2e-4)
VCLIP_BAND = 5e-2  # |V - V_old| against clip_vloss_coef


def n_relu(name):
    """ReLU calls of one forward of the network: two per block, one per hidden layer of the encoder"""
    s = spec(name)
    return 0 if s.activation != "ReLU" else len(s.mlp_dims) - 1 + (len(s.cond_mlp_dims) - 1 if s.cond_mlp_dims else 0)


def relu_row(name):
    return n_relu(name) > 0


def _mse_draw(s, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(n, s.horizon_steps, s.action_dim, generator=gen) * 2 - 1, torch.rand(n, 1, s.cond_dim, generator=gen) * 2 - 1,
            torch.randint(0, K, (n,), generator=gen), torch.randn(n, s.horizon_steps, s.action_dim, generator=gen))


def _clear_rows(margins, n):
    """the first n rows of a pool whose smallest |ReLU input| (float64 oracle) is at least twice the band"""
    keep = torch.nonzero(margins >= 2 * RELU_BAND).reshape(-1)
    assert len(keep) >= n, (len(keep), n)
    return keep[:n]


@functools.lru_cache(maxsize=None)
def mse_inputs(name, N):
    """(x0, state, t, noise): for a ReLU network the first N rows of a pool of 2 N + 8 that keep every ReLU input of the float64
    oracle clear of zero -- rows are independent, so the choice is judged by the oracle alone, row by row (as POOLED does in
    tests/test_unet_specs.py)"""
    s = spec(name)
    if not relu_row(name):
        return _mse_draw(s, N, 300 + N)
    x0, state, t, noise = _mse_draw(s, 2 * N + 8, 300 + N)
    log = []
    with torch.no_grad(), oracle_mode(relu_log=log):
        O.denoise_mse_loss(K, s, params(s, SEED_MSE, F64), x0.double(), state.double(), t, noise.double())
    keep = _clear_rows(torch.stack(log).amin(dim=0), N)
    return x0[keep], state[keep], t[keep], noise[keep]


def _grads(prm):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in prm.items()}


@functools.lru_cache(maxsize=None)
def ref_mse(name, N, mode="f64"):
    """(loss, {parameter: gradient}, smallest |ReLU input| or None)"""
    s = spec(name)
    dtype, rounded = MODES[mode]
    x0, state, t, noise = mse_inputs(name, N)
    prm = {k: v.requires_grad_(True) for k, v in params(s, SEED_MSE, dtype).items()}
    log = []
    with oracle_mode(rounded, relu_log=log):
        loss = O.denoise_mse_loss(K, s, prm, x0.to(dtype), state.to(dtype), t, noise.to(dtype))
        loss.backward()
    return float(loss.detach()), _grads(prm), (float(torch.stack(log).min()) if log else None)


# ------------------------------------------------------------------ the PPO update
# One case: actor row, critic row, R rollouts, Kft fine-tuned steps (of K = 2 Kft), M minibatch samples out of the R * Kft, options.
# The actor's and the critic's backward both see M rows.  Every actor row runs a tiny minibatch and one that reaches its route
# (M >= 100 out_dim for the low-rank top where the row has one); every critic row runs, c256_in32 on both sides of M = 100.
def _case(actor, critic, R, Kft, M=None, **opt):
    if critic == "std":
        critic = f"std{EDGE_ACTORS[actor]['cond_dim']}"
    return (actor, critic, R, Kft, R * Kft if M is None else M, tuple(sorted(opt.items())))


PPO_CASES = [
    _case("h128_out1", "c128_nb0", 8, 10), _case("h128_out1", "c128_nb0", 130, 10),
    _case("h384_nb2", "std", 8, 10), _case("h384_nb2", "std", 130, 10),
    _case("h768", "std", 8, 10), _case("h768", "std", 130, 25),
    _case("h1152", "c768", 8, 10), _case("h1152", "c768", 130, 10),
    _case("h256_nb0", "c768", 8, 10), _case("h256_nb0", "c512_ln_nb2", 130, 10),
    _case("h256_nb2", "c512_ln_nb2", 8, 10), _case("h256_nb2", "c512_ln_nb2", 130, 10, norm_adv=False),
    _case("h256_ln_nb8", "std", 8, 10), _case("h256_ln_nb8", "std", 130, 10, M=599),
    _case("h512_ln_nb2", "c512_ln_nb2", 8, 10), _case("h512_ln_nb2", "c768", 130, 10, M=1200),
    _case("h512_out16", "std", 8, 10), _case("h512_out16", "std", 130, 25, M=1599), _case("h512_out16", "std", 130, 25, M=1600),
    _case("h512_out17", "std", 8, 10), _case("h512_out17", "std", 130, 25),
    _case("h512_out64", "std", 8, 10), _case("h512_out64", "std", 1300, 10),
    _case("h512_out65", "std", 8, 10), _case("h512_out65", "std", 1300, 10),
    _case("h512_out128", "std", 8, 10), _case("h512_out128", "std", 130, 10), _case("h512_out128", "std", 1280, 10),
    _case("h256_room", "std", 8, 10), _case("h256_room", "std", 130, 10), _case("h256_room", "std", 130, 25),
    _case("h256_round", "std", 8, 10), _case("h256_round", "std", 130, 10, vclip=0.2),
    _case("h256_noroom", "std", 8, 10), _case("h256_noroom", "std", 130, 10, quantiles=(0.1, 0.9)),
    _case("h256_af3", "std", 8, 10), _case("h256_af3", "std", 130, 10),
    _case("h256_td36", "std", 8, 10), _case("h256_td36", "std", 130, 10),
    _case("h256_enc8", "std", 8, 10), _case("h256_enc8", "std", 130, 10),
    _case("h256_enc16", "std", 8, 10), _case("h256_enc16", "std", 130, 10),
    _case("h256_in320", "std", 8, 10), _case("h256_in320", "std", 130, 10),
    _case("h1024_in1024", "std", 8, 10), _case("h1024_in1024", "std", 130, 10),
    _case("h256_c32", "c256_in32", 10, 10, M=99), _case("h256_c32", "c256_in32", 10, 10, M=100), _case("h256_c32", "c256_in32", 130, 10),
    _case("h256_c33", "c256_in33", 8, 10), _case("h256_c33", "c256_in33", 130, 10),
    _case("h256_enc_c1024", "c1024_in1024", 8, 10), _case("h256_enc_c1024", "c1024_in1024", 130, 10),
]
BC_CASE = ("h256_room", 40, 10)  # the behaviour-cloning term: actor row, B observations, Kft (M = 400 rows >= 100 out_dim)
BC_MIX = 0.02  # its fine-tuned network sits this close to the base network, so that no log-prob of the base chains is in the tail


def case_id(c):
    return f"{c[0]}-{c[1]}-R{c[2]}-Kft{c[3]}-M{c[4]}" + "".join(f"-{k}" for k, _ in c[5])


def ppo_kw(case):
    opt = dict(case[5])
    kw = dict(denoising_steps=2 * case[3], ft_denoising_steps=case[3], randn_clip_value=2.5, gamma_denoising=0.99,
              clip_ploss_coef=0.1, clip_ploss_coef_base=0.02, norm_adv=opt.get("norm_adv", True))
    if "vclip" in opt:
        kw["clip_vloss_coef"] = opt["vclip"]
    if "quantiles" in opt:
        kw["clip_advantage_lower_quantile"], kw["clip_advantage_upper_quantile"] = opt["quantiles"]
    return kw


def _x0_margin(cfg, s, ft, prev, t, state):
    """per sample: how far the float64 oracle's x0 prediction stays from the +-denoised_clip_value clamp (DDPM)"""
    with torch.no_grad():
        eps = O.actor_forward(ft, s, prev, t, state)
    tab = cfg.tables
    x0 = O._col(tab["sqrt_recip_alphas_cumprod"], t) * prev - O._col(tab["sqrt_recipm1_alphas_cumprod"], t) * eps
    return (x0.abs() - cfg.denoised_clip_value).abs().reshape(len(t), -1).amin(dim=1)


TINY, DRAWS = 200, 4


@functools.lru_cache(maxsize=None)
def ppo_draw(case):
    """Which of DRAWS independent draws of a tiny minibatch (M < TINY) the tests use: the best-conditioned one, judged by the oracle
    alone.  With 80 samples, half of them clipped and ten steps, a small gradient tensor is a sum of a few dozen terms of both
    signs -- the out-layer bias gradient of h128_out1's first draw cancels 91-fold (sum |terms| / |sum|), so that the 0.2 % a
    bf16 forward costs each term is anything up to 4.6 % of the sum -- and what such a sum loses to rounding is luck, for the
    rounded oracle as for a kernel.  The draw taken is the one whose worst gradient check, rounded oracle against float64
    oracle in units of the usual bf16 bounds, is smallest."""
    if case[4] >= TINY:
        return 0

    def score(draw):
        want, got = _ref_ppo(case, "f64", draw), _ref_ppo(case, "bf16ops", draw)
        checks = dict(grad_checks(got[1], want[1], "bf16", "actor"), **grad_checks(got[2], want[2], "bf16", "critic"))
        return max(v / b for v, b in checks.values())
    return min(range(DRAWS), key=score)


def ppo_batch(case):
    return _ppo_batch(case, ppo_draw(case))


def ref_ppo(case, mode="f64"):
    return _ref_ppo(case, mode, ppo_draw(case))


@functools.lru_cache(maxsize=None)
def _ppo_batch(case, draw):
    """A rollout buffer of R observations whose chains are the FLOAT64 oracle's own (rounded to float32, as the HIP path is
    handed them), with old log-probs = the float64 oracle's + a per-sample shift that puts half the samples well inside the clip
    range and half well outside.  The R rollouts are the first of a pool (1.25 R + 8; 5 R + 16 with a ReLU network: 25 steps x
    1024 inputs of order 0.3 leave one rollout in three clear) whose Kft samples keep every ReLU input of the fine-tuned actor
    and of the critic, and every x0 clamp of the float64 oracle, 1.5 bands from the kink.  (The frozen network's forward runs
    on the same rows and is overwritten row for row: it carries no gradient and takes no part.)"""
    aname, cname, R, Kft, M, _ = case
    a, c = spec(aname), spec(cname)
    cfg = make_cfg(a, ppo_kw(case))
    Ta, Da = a.horizon_steps, a.action_dim
    P = 5 * R + 16 if relu_row(aname) or relu_row(cname) else R + R // 4 + 8
    gen = torch.Generator().manual_seed(17 * R + Kft + 1000 * draw)
    state = torch.rand(P, 1, a.cond_dim, generator=gen) * 2 - 1
    noise = torch.randn(cfg.denoising_steps + 1, P, Ta, Da, generator=gen)
    base, ft, cr = params(a, SEED_BASE, F64), ft_params(a, F64), params(c, SEED_CRITIC, F64)
    log_a, log_c = [], []
    with oracle_mode():
        chains = O.sample_chain(cfg, a, base, ft, state.double(), noise.double())[1].float()
        with torch.no_grad(), oracle_mode(relu_log=log_a):
            lp = O.chain_logprob(cfg, a, base, ft, state.double(), chains.double()).reshape(P, Kft, Ta, Da)
        with torch.no_grad(), oracle_mode(relu_log=log_c):
            val = O.critic_forward(cr, c, state.double()).reshape(P)
        kk = torch.arange(Kft).repeat(P)
        x0m = _x0_margin(cfg, a, ft, chains[:, :-1].reshape(-1, Ta, Da).double(), O._ft_time_indices(cfg)[0][kk],
                         O._repeat_rows(state.double(), Kft)).reshape(P, Kft).amin(dim=1)
    ok = x0m >= 1.5 * CLAMP_BAND
    assert len(log_a) == 2 * n_relu(aname) and len(log_c) == n_relu(cname)
    for m in log_a[n_relu(aname):] + log_c:
        ok &= m.reshape(P, -1).amin(dim=1) >= 1.5 * RELU_BAND
    keep = torch.nonzero(ok).reshape(-1)
    assert len(keep) >= R, (case_id(case), len(keep))
    keep = keep[:R]
    state, chains, lp, val = state[keep], chains[keep], lp[keep], val[keep]
    inside = torch.rand(R, Kft, generator=gen) < 0.5
    mag = torch.where(inside, torch.rand(R, Kft, generator=gen) * 0.01, 0.15 + 0.1 * torch.rand(R, Kft, generator=gen))
    delta = mag * (torch.randint(0, 2, (R, Kft), generator=gen) * 2 - 1)
    oldlp = (lp + delta.double().reshape(R, Kft, 1, 1)).float()
    far = torch.randint(0, 2, (R,), generator=gen).bool()  # value clip (where a case has one): half the rows clipped
    dv = torch.where(far, torch.full((R,), 0.4), torch.full((R,), 0.05)) * (torch.randint(0, 2, (R,), generator=gen) * 2 - 1)
    oldv = (val + dv.double()).float()
    # returns above the value by 0.25 .. 0.8: the critic's bias gradients are sums without cancellation, and the clipped value
    # loss's max() never ties (with V - V_old = +-0.4 it would at V_ret - V = -+0.1)
    ret = (val + (0.25 + 0.55 * torch.rand(R, generator=gen)).double()).float()
    adv = 0.3 + 2.0 * torch.randn(R, generator=gen)
    inds = torch.randperm(R * Kft, generator=gen)[:M]
    return dict(state=state, chains=chains, oldlp=oldlp, oldv=oldv, ret=ret, adv=adv, inds=inds,
                reward_horizon=min(4, Ta))


STAT_NAMES = ("pg_loss", "v_loss", "approx_kl", "clipfrac", "ratio")


@functools.lru_cache(maxsize=None)
def _ref_ppo(case, mode, draw):
    """(the five statistics in the library's order, actor gradients of pg_loss, critic gradients of v_loss, margins), numpy"""
    aname, cname, R, Kft, M, _ = case
    a, c = spec(aname), spec(cname)
    dtype, rounded = MODES[mode]
    cfg = make_cfg(a, ppo_kw(case))
    b = _ppo_batch(case, draw)
    rows, kk = b["inds"] // Kft, b["inds"] % Kft
    ft = {k: v.requires_grad_(True) for k, v in ft_params(a, dtype).items()}
    cr = {k: v.requires_grad_(True) for k, v in params(c, SEED_CRITIC, dtype).items()}
    f = lambda x: x.to(dtype)
    log = []
    with oracle_mode(rounded, relu_log=log):
        res = O.ppo_loss(cfg, a, c, params(a, SEED_BASE, dtype), ft, cr, f(b["state"][rows]), f(b["chains"][rows, kk]),
                         f(b["chains"][rows, kk + 1]), kk, f(b["ret"][rows]), f(b["oldv"][rows]), f(b["adv"][rows]),
                         f(b["oldlp"][rows, kk]), reward_horizon=b["reward_horizon"])
        (res[0] + res[2]).backward()
        margins = {}
        if mode == "f64":  # the decisions of THIS evaluation, recomputed from its own quantities
            with torch.no_grad():
                lp, _ = O.logprob_subsample(cfg, a, params(a, SEED_BASE, dtype), ft, f(b["state"][rows]), f(b["chains"][rows, kk]),
                                            f(b["chains"][rows, kk + 1]), kk)
                old = f(b["oldlp"][rows, kk])
                rh = b["reward_horizon"]
                ratio = (lp.clamp(-5, 2)[:, :rh].mean(dim=(-1, -2)) - old.clamp(-5, 2)[:, :rh].mean(dim=(-1, -2))).exp()
                eps_k = O.clip_coef_schedule(cfg, kk).double()
                newv = O.critic_forward(cr, c, f(b["state"][rows])).view(-1)
            live = log[n_relu(aname):2 * n_relu(aname) + n_relu(cname)]  # the loss's own calls, without the frozen network's forward
            margins["relu"] = float(torch.stack([m.min() for m in live]).min()) if live else None
            margins["logprob_clamp"] = float(min((x - bound).abs().min() for x in (lp, old) for bound in (-5.0, 2.0)))
            margins["ratio_clip"] = float(((ratio - 1).abs() - eps_k).abs().min())
            margins["x0_clamp"] = float(_x0_margin(cfg, a, ft, f(b["chains"][rows, kk]), O._ft_time_indices(cfg)[0][kk],
                                                   f(b["state"][rows])).min())
            margins["clipped"] = float(((ratio - 1).abs() > eps_k).double().mean())
            margins["ratio_dev"] = float((ratio - 1).abs().mean())
            if cfg.clip_vloss_coef is not None:
                d = newv - f(b["oldv"][rows])
                margins["value_clip"] = float((d.abs() - cfg.clip_vloss_coef).abs().min())
                vcl = f(b["oldv"][rows]) + d.clamp(-cfg.clip_vloss_coef, cfg.clip_vloss_coef)
                margins["value_max"] = float(((newv - f(b["ret"][rows])).abs() - (vcl - f(b["ret"][rows])).abs()).abs()[d.abs() > cfg.clip_vloss_coef].min())
    stats = np.array([res[0].item(), res[2].item(), res[4], res[3], res[5]], dtype=np.float64)
    return stats, _grads(ft), _grads(cr), margins


BC_KW = dict(denoising_steps=2 * BC_CASE[2], ft_denoising_steps=BC_CASE[2], randn_clip_value=2.5, gamma_denoising=0.99,
             clip_ploss_coef=0.1)


@functools.lru_cache(maxsize=None)
def bc_inputs():
    """(observations, noise): the first B of a pool of 5 B + 16 observations whose Kft scored rows keep every ReLU input of the
    fine-tuned network and every x0 clamp of the float64 oracle 1.5 bands from the kink (as ppo_batch does)"""
    name, B, Kft = BC_CASE
    s = spec(name)
    P = 5 * B + 16
    gen = torch.Generator().manual_seed(91)
    state = torch.rand(P, 1, s.cond_dim, generator=gen) * 2 - 1
    noise = torch.randn(2 * Kft + 1, P, s.horizon_steps, s.action_dim, generator=gen)
    cfg = make_cfg(s, BC_KW)
    base, ft = params(s, SEED_BASE, F64), ft_params(s, F64, BC_MIX)
    log = []
    with oracle_mode():
        chains = O.sample_chain(cfg, s, base, ft, state.double(), noise.double(), use_base_policy=True)[1]
        with torch.no_grad(), oracle_mode(relu_log=log):
            O.chain_logprob(cfg, s, base, ft, state.double(), chains)
        x0m = _x0_margin(cfg, s, ft, chains[:, :-1].reshape(-1, s.horizon_steps, s.action_dim), O._ft_time_indices(cfg)[0][torch.arange(Kft).repeat(P)],
                         O._repeat_rows(state.double(), Kft)).reshape(P, Kft).amin(dim=1)
    ok = x0m >= 1.5 * CLAMP_BAND
    for m in log[n_relu(name):]:
        ok &= m.reshape(P, -1).amin(dim=1) >= 1.5 * RELU_BAND
    keep = torch.nonzero(ok).reshape(-1)[:B]
    assert len(keep) == B
    return state[keep], noise[:, keep].contiguous()


@functools.lru_cache(maxsize=None)
def ref_bc(mode="f64"):
    """(bc_loss, gradients, margins) of O.bc_loss on the recorded noise"""
    name = BC_CASE[0]
    s = spec(name)
    dtype, rounded = MODES[mode]
    cfg = make_cfg(s, BC_KW)
    state, noise = bc_inputs()
    base = params(s, SEED_BASE, dtype)
    ft = {k: v.requires_grad_(True) for k, v in ft_params(s, dtype, BC_MIX).items()}
    log = []
    with oracle_mode(rounded, relu_log=log):
        loss, chains = O.bc_loss(cfg, s, base, ft, state.to(dtype), noise.to(dtype))
        loss.backward()
        with torch.no_grad():
            lp = O.chain_logprob(cfg, s, base, ft, state.to(dtype), chains)
    margins = dict(relu=float(torch.stack([m.min() for m in log[-n_relu(name):]]).min()),  # (the fine-tuned network's scoring pass)
                   logprob_clamp=float(min((lp - bound).abs().min() for bound in (-5.0, 2.0))))
    return float(loss.detach()), _grads(ft), margins


# ------------------------------------------------------------------ 1. the routes the GPU tests take, as a literal table
def _r(s):
    return frozenset(s.split(",")) - {""}


# (row, precision, M, Kft, flags) -> route.  Actors: the PPO update passes ZEROED | SIDE, the denoising loss SIDE with Kft = K.
ROUTES = {}


def used_routes():
    """every (row, precision, M, Kft, flags) the GPU tests below run a backward at"""
    keys = set()
    for prec in ("fp32", "bf16"):
        for name in ACTOR_NAMES:
            for N in MSE_BATCHES:
                keys.add((name, prec, N, K, SIDE))
        for aname, cname, R, Kft, M, _ in PPO_CASES:
            keys.add((aname, prec, M, Kft, PPO_ACTOR))
            keys.add((cname, prec, M, Kft, PPO_CRITIC))
        keys.add((BC_CASE[0], prec, BC_CASE[1] * BC_CASE[2], BC_CASE[2], SIDE))
    return keys


def _routes(name, flags, rows):
    """rows: (precision or "*" for both, M or a tuple of them, Kft, the bits set)"""
    for prec, Ms, Kft, r in rows:
        for p in (("fp32", "bf16") if prec == "*" else (prec,)):
            for M in (Ms if isinstance(Ms, tuple) else (Ms,)):
                assert (name, p, M, Kft, flags) not in ROUTES
                ROUTES[(name, p, M, Kft, flags)] = _r(r)


FM = "fused,merged"
ONE = "fused,one_block,lowrank"  # a one-block network on its own backward kernel: M >= 100 out_dim
ONEM = ONE + ",merged"           # ... with the merged forward
# -- critics in the PPO update (ZEROED); std<n>: the usual [256] * 3 Mish critic on n observation columns
_routes("c128_nb0", PPO_CRITIC, [("*", (80, 1300), 10, "")])
_routes("c256_in32", PPO_CRITIC, [("*", 99, 10, FM + ",post_one"), ("fp32", (100, 1300), 10, ONEM + ",post_one"),
                                  ("bf16", (100, 1300), 10, ONEM + ",dw0,post_one")])
_routes("c256_in33", PPO_CRITIC, [("*", 80, 10, FM + ",post_one"), ("*", 1300, 10, ONEM + ",post_one")])
_routes("c512_ln_nb2", PPO_CRITIC, [("*", 80, 10, "fused"), ("*", 1300, 10, "fused,lowrank,post_one")])
_routes("c768", PPO_CRITIC, [("*", 80, 10, ""), ("*", (1200, 1300), 10, "lowrank,post_one")])
_routes("c1024_in1024", PPO_CRITIC, [("*", 80, 10, "fused"), ("*", 1300, 10, ONE + ",post_one")])
for _n in ("std1004", "std300"):  # Kp0 > hidden: layered, though one_block is reported
    _routes(_n, PPO_CRITIC, [("*", 80, 10, ""), ("*", 1300, 10, "one_block,lowrank,post_one")])
for _n in ("std19", "std20", "std5"):
    _routes(_n, PPO_CRITIC, [("*", 80, 10, FM + ",post_one"), ("fp32", 1300, 10, ONEM + ",post_one"),
                             ("bf16", 1300, 10, ONEM + ",dw0,post_one")])
_routes("std7", PPO_CRITIC, [("*", 80, 10, FM + ",post_one"), ("fp32", 599, 10, ONEM + ",post_one"), ("bf16", 599, 10, ONEM + ",dw0,post_one")])
_routes("std8", PPO_CRITIC, [("*", 80, 10, FM + ",post_one"), ("fp32", (1300, 12800, 13000), 10, ONEM + ",post_one"),
                             ("bf16", (1300, 12800, 13000), 10, ONEM + ",dw0,post_one"),
                             ("fp32", (1599, 1600, 3250), 25, ONEM + ",post_one"), ("bf16", (1599, 1600, 3250), 25, ONEM + ",dw0,post_one")])
_routes("std9", PPO_CRITIC, [("*", 80, 10, FM + ",post_one"), ("fp32", 3250, 25, ONEM + ",post_one"), ("bf16", 3250, 25, ONEM + ",dw0,post_one")])
# -- actors in the denoising loss (SIDE; Kft = K = 20 one-hot columns) and in the behaviour-cloning term (h256_room, M = 400)
for _n in ("h1024_in1024", "h256_ln_nb8", "h256_nb0", "h256_nb2", "h512_ln_nb2", "h512_out128", "h512_out65"):
    _routes(_n, SIDE, [("*", (12, 130), 20, "fused,onehot")])
for _n in ("h1152", "h256_in320", "h384_nb2", "h768"):  # the layered chain (FUSED clear: no other bit means anything)
    _routes(_n, SIDE, [("*", (12, 130), 20, "need_aux")])
_routes("h128_out1", SIDE, [("*", 12, 20, "need_aux"), ("*", 130, 20, "lowrank,need_aux,post_one")])
for _n in ("h256_af3", "h256_c32", "h256_c33", "h256_enc16", "h256_enc_c1024", "h256_noroom", "h256_round", "h256_td36", "h512_out17"):
    _routes(_n, SIDE, [("*", (12, 130), 20, FM + ",onehot")])
_routes("h256_enc8", SIDE, [("*", (12, 130), 20, FM + ",need_aux,post_one")])
_routes("h256_room", SIDE, [("*", (12, 130), 20, FM + ",onehot"), ("*", 400, 10, ONEM + ",onehot")])
for _n in ("h512_out16", "h512_out64"):  # fused_can_merge: bf16 yes, fp32 no
    _routes(_n, SIDE, [("fp32", (12, 130), 20, "fused,onehot"), ("bf16", (12, 130), 20, FM + ",onehot")])
# -- actors in the PPO update (ZEROED | SIDE)
_routes("h1024_in1024", PPO_ACTOR, [("*", 80, 10, "fused,onehot,post_one"), ("*", 1300, 10, ONE + ",onehot,post_one")])
for _n in ("h1152", "h128_out1", "h384_nb2"):
    _routes(_n, PPO_ACTOR, [("*", 80, 10, "need_aux"), ("*", 1300, 10, "lowrank,need_aux,post_one")])
_routes("h768", PPO_ACTOR, [("*", 80, 10, "need_aux"), ("*", 3250, 25, "lowrank,need_aux,post_one")])
_routes("h256_in320", PPO_ACTOR, [("*", 80, 10, "need_aux"), ("*", 1300, 10, "one_block,lowrank,need_aux,post_one")])
for _n in ("h256_af3", "h256_c33", "h256_enc16", "h256_enc_c1024", "h256_noroom", "h256_td36"):
    _routes(_n, PPO_ACTOR, [("*", 80, 10, FM + ",onehot,post_one"), ("*", 1300, 10, ONEM + ",onehot,post_one")])
_routes("h256_c32", PPO_ACTOR, [("*", (99, 100), 10, FM + ",onehot,post_one"), ("*", 1300, 10, ONEM + ",onehot,post_one")])
_routes("h256_enc8", PPO_ACTOR, [("*", 80, 10, FM + ",need_aux,post_one"), ("*", 1300, 10, ONEM + ",need_aux,post_one")])
_routes("h256_ln_nb8", PPO_ACTOR, [("*", (80, 599), 10, "fused,onehot,post_one")])
_routes("h256_nb0", PPO_ACTOR, [("*", (80, 1300), 10, "fused,onehot,post_one")])
_routes("h256_nb2", PPO_ACTOR, [("*", 80, 10, "fused,onehot,post_one"), ("*", 1300, 10, "fused,lowrank,onehot,post_one")])
_routes("h256_room", PPO_ACTOR, [("*", 80, 10, FM + ",onehot,post_one"), ("fp32", 1300, 10, ONEM + ",onehot,post_one"),
                                 ("bf16", 1300, 10, ONEM + ",onehot,dw0,dw0_nhot,side_tail,tail_post,post_one"),
                                 ("*", 3250, 25, ONEM + ",onehot,post_one")])  # (25 one-hot columns, room for 20: no dW0)
_routes("h256_round", PPO_ACTOR, [("*", 80, 10, FM + ",onehot,post_one"), ("fp32", 1300, 10, ONEM + ",onehot,post_one"),
                                  ("bf16", 1300, 10, ONEM + ",onehot,dw0,dw0_nhot,dw0_round,side_tail,tail_post,post_one")])
_routes("h512_ln_nb2", PPO_ACTOR, [("*", 80, 10, "fused,onehot,post_one"), ("*", 1200, 10, "fused,lowrank,onehot,post_one")])
_routes("h512_out128", PPO_ACTOR, [("*", (80, 1300), 10, "fused,onehot,post_one"), ("*", 12800, 10, ONE + ",onehot,post_one")])
_routes("h512_out16", PPO_ACTOR, [("fp32", 80, 10, "fused,onehot,post_one"), ("bf16", 80, 10, FM + ",onehot,post_one"),
                                  ("fp32", 1599, 25, "fused,onehot,post_one"), ("bf16", 1599, 25, FM + ",onehot,post_one"),
                                  ("fp32", 1600, 25, ONE + ",onehot,post_one"), ("bf16", 1600, 25, ONEM + ",onehot,post_one")])
_routes("h512_out17", PPO_ACTOR, [("*", 80, 10, FM + ",onehot,post_one"), ("*", 3250, 25, ONEM + ",onehot,post_one")])
_routes("h512_out64", PPO_ACTOR, [("fp32", 80, 10, "fused,onehot,post_one"), ("bf16", 80, 10, FM + ",onehot,post_one"),
                                  ("fp32", 13000, 10, ONE + ",onehot,post_one"), ("bf16", 13000, 10, ONEM + ",onehot,post_one")])
_routes("h512_out65", PPO_ACTOR, [("*", 80, 10, "fused,onehot,post_one"), ("*", 13000, 10, ONE + ",onehot,post_one")])
BF16_ONLY_BITS = {"dw0", "dw0_nhot", "dw0_round", "side_tail", "tail_post"}  # plan_route(): R.dw0 needs P::ESIZE == 2, the rest need R.dw0


def test_every_route_the_gpu_tests_take_is_pinned_and_every_bit_shows_both_ways():
    """dppo_backward_route (host code, no GPU) for every (row, precision, rows, Kft, flags) a backward of this file runs at,
    against the literal table above; then, over the table: each of the twelve route bits occurs set and clear in each precision
    that can set it (the in-kernel dW0 and what hangs on it are bf16-only by construction: plan_route() asks P::ESIZE == 2),
    both forms of the merged forward (out_dim <= 16, and 17 .. 64) take the one-block route, and the M = 100 out_dim threshold
    of the low-rank top is met one below and exactly on, for an actor and for a critic.  Removing a row or a case from this
    file fails here."""
    used = used_routes()
    assert used == set(ROUTES), (sorted(used - set(ROUTES)), sorted(set(ROUTES) - used))
    for key in sorted(ROUTES):
        name, prec, M, Kft, flags = key
        assert route(actor_desc(name), prec, M, flags, Kft) == ROUTES[key], key
    for prec in ("fp32", "bf16"):
        seen = [r for k, r in ROUTES.items() if k[1] == prec]
        for bit in BITS:
            if prec == "fp32" and bit in BF16_ONLY_BITS:
                assert not any(bit in r for r in seen), bit
            else:
                assert any(bit in r for r in seen) and any(bit not in r for r in seen), (prec, bit)
        merged_one = {spec(k[0]).out_dim for k, r in ROUTES.items() if k[1] == prec and {"merged", "one_block"} <= r}
        assert any(o <= 16 for o in merged_one) and any(17 <= o <= 64 for o in merged_one), (prec, merged_one)
        for name, flags in (("h512_out16", PPO_ACTOR), ("c256_in32", PPO_CRITIC)):
            edge = 100 * spec(name).out_dim
            below = [r for k, r in ROUTES.items() if k[:3] == (name, prec, edge - 1) and k[4] == flags]
            on = [r for k, r in ROUTES.items() if k[:3] == (name, prec, edge) and k[4] == flags]
            assert below and on and not {"lowrank", "one_block"} & below[0] and {"lowrank", "one_block"} <= on[0], (name, prec)
    # every row of both tables runs, every critic row in the PPO update
    assert {k[0] for k in ROUTES if not k[0].startswith("std")} == set(ACTOR_NAMES) | set(CRITIC_NAMES)
    assert {c[0] for c in PPO_CASES} == set(ACTOR_NAMES) and {c[1] for c in PPO_CASES} >= set(CRITIC_NAMES)
    assert all(spec(c[0]).cond_dim == spec(c[1]).cond_dim for c in PPO_CASES)  # the critic reads the actor's observation
    for opt in ("norm_adv", "vclip", "quantiles"):
        assert sum(opt in dict(c[5]) for c in PPO_CASES) == 1, opt


# ------------------------------------------------------------------ 5. bounds: every check is a dict {quantity: (distance, bound)}
# fp32: tests/test_hip_parity.py (forward 2e-5, chains 1e-4, log-probs 2e-4 and 1e-4 in the mean, loss and statistics 2e-4 relative
# with the 2e-6 floor of test_tiny_and_ragged_minibatches_match_oracle, gradients rtol 2e-3 with atol 2e-4 |g| / sqrt(n) + 1e-7).
# bf16: tests/test_hip_parity.py (forward 3e-2, chains 5e-2, log-probs 0.6 and 0.06 in the mean, denoising loss 2e-2) and
# tests/test_bf16_parity.py (pg_loss 1e-4 abs, v_loss 2e-3 rel, approx_kl 2e-6 abs for ratios near 1, grown by 2e-4 mean |ratio - 1|
# for the ratios of this file as scalar_checks() derives, ratio 2e-4 abs, bc_loss 5e-3 rel; clipfrac
# to less than half a sample, 0.5 / M: RATIO_BAND keeps every sample on its side, and the library forms the fraction in
# float32), per-tensor gradient cosine >= 0.99 and norm within 3 %.
def ac(got, want):
    """max |got - want| / (1 + |want|): <= tol is what assert_allclose(rtol=tol, atol=tol) asks"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max())


def scalar_checks(kind, got, want, prec, scale=1.0, ratio_dev=0.0, M=1):
    """scale < 1: the float32 oracle against the float64 one at that fraction of the fp32 bounds.  ratio_dev: the reference's
    mean |ratio - 1|.  approx_kl = mean((r - 1) - log r) moves by (r - 1) d for an error d of the log-ratio, and
    tests/test_bf16_parity.py holds the ratio to 2e-4: its 2e-6 (for ratios within 1e-2 of 1) grows by 2e-4 mean |r - 1| here,
    where half the samples sit 0.14 .. 0.28 outside: 1.9e-5 .. 2.8e-5 on the minibatches of this file (measured on an MI355X:
    at most 6.8e-6, h512_ln_nb2 at M = 80)."""
    f = prec == "fp32"
    rel = lambda x, y, floor=0.0: abs(x - y) / (abs(y) + floor)
    if kind == "forward":
        return {"forward": (ac(got, want), 2e-5 * scale if f else 3e-2)}
    if kind == "chain":
        return {"chains": (ac(got[0], want[0]), 1e-4 * scale if f else 5e-2), "trajectories": (ac(got[1], want[1]), 1e-4 * scale if f else 5e-2)}
    if kind == "logprob":
        return {"logprob": (ac(got, want), 2e-4 * scale if f else 0.6),
                "logprob_mean": (float(np.abs(np.asarray(got, np.float64) - want).mean()), 1e-4 * scale if f else 0.06)}
    if kind == "mse":
        return {"loss": (rel(got, want), 2e-4 * scale if f else 2e-2)}
    if kind == "bc":
        return {"bc_loss": (rel(got, want, 1e-2), 2e-4 * scale if f else 5e-3)}
    assert kind == "ppo"
    if f:
        return {n: (rel(got[i], want[i], 1e-2), 2e-4 * scale) for i, n in enumerate(STAT_NAMES)}
    return {"pg_loss": (abs(got[0] - want[0]), 1e-4), "v_loss": (rel(got[1], want[1]), 2e-3), "approx_kl": (abs(got[2] - want[2]), 2e-6 + 2e-4 * ratio_dev),
            "clipfrac": (abs(got[3] - want[3]), 0.5 / M), "ratio": (abs(got[4] - want[4]), 2e-4)}


def grad_checks(got, want, prec, tag, scale=1.0):
    """got, want: {parameter: array} in one order; no reference tensor may be zero (a skipped tensor would pass 0 / 0)"""
    assert list(got) == list(want)
    out = {}
    for k, w in want.items():
        g, w = np.asarray(got[k], np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), (tag, k)
        nw = float(np.linalg.norm(w))
        assert nw > 0, (tag, k)
        if prec == "fp32":
            atol = (2e-4 * nw / math.sqrt(w.size) + 1e-7) * scale
            out[f"{tag}.{k}"] = (float((np.abs(g - w) / (atol + 2e-3 * scale * np.abs(w))).max()), 1.0)
        else:
            c, r = cos_ratio(g, w)
            out[f"{tag}.{k} cosine"] = (1.0 - c, 0.01)
            out[f"{tag}.{k} norm"] = (abs(r - 1.0), 0.03)
    return out


# Rows whose bf16 bounds come from the rounded oracle: where bf16 OPERANDS alone (the float64 oracle with every Linear's weights,
# input and output gradient rounded through bfloat16; no kernel) already use more than half of a bound, that bound becomes twice
# the rounded oracle's distance.  test_bf16_bounds_from_the_rounded_oracle_are_needed holds the list to exactly those rows.
BF16_FROM_ROUNDED_ORACLE = {"h1152", "h128_out1", "h256_af3", "h256_ln_nb8", "h256_nb0", "h256_room", "h256_round", "h384_nb2", "h512_ln_nb2",
                            "h512_out64", "h512_out65", "h768"}


def judge(row, prec, checks, yard=None, what=""):
    """Print every figure, then assert.  yard: () -> the same checks for the rounded oracle (bf16 rows of the list only)."""
    bad, worst, units = [], ("", 0.0), ("", 0.0)
    y = yard() if prec == "bf16" and row in BF16_FROM_ROUNDED_ORACLE and yard is not None else {}
    for k, (v, b) in checks.items():
        if k in y and 2 * y[k][0] > b:
            units = max(units, (k, v / y[k][0]), key=lambda t: t[1])
            b = 2 * y[k][0]
        worst = max(worst, (k, v / b if b > 0 else (0.0 if v == 0 else float("inf"))), key=lambda t: t[1])
        if not v <= b:
            bad.append((k, v, b))
    print(f"{what} {prec}: worst {worst[0]} at {worst[1]:.3f} of its bound"
          + (f"; worst in units of the bf16-operand yardstick {units[0]} {units[1]:.2f} (2 is the bound)" if units[0] else ""))
    assert not bad, (what, prec, bad)


# ------------------------------------------------------------------ 3. CPU: the reference itself
def fwd_checks(name, get, prec, scale=1.0):
    """get(B) -> the network's output on fwd_inputs(name, B)"""
    return {f"B={B} {k}": v for B in FWD_BATCHES for k, v in scalar_checks("forward", get(B), ref_forward(name, B), prec, scale).items()}


def chain_checks(name, cm, B, got, prec, scale=1.0):
    """got: (chains or None where the sampler refuses, trajectories, log-probs of the float64 oracle's chains)"""
    want = ref_chain(name, cm, B)
    out = {} if got[0] is None else scalar_checks("chain", got[:2], want[:2], prec, scale)
    out.update(scalar_checks("logprob", got[2], want[2], prec, scale))
    return {f"{cm} B={B} {k}": v for k, v in out.items()}


def mse_checks(name, N, got, prec, scale=1.0):
    want = ref_mse(name, N)
    out = {f"mse N={N} {k}": v for k, v in scalar_checks("mse", got[0], want[0], prec, scale).items()}
    out.update(grad_checks(got[1], want[1], prec, f"mse N={N}", scale))
    return out


def all_checks(name, mode, prec, scale=1.0):
    """every check of every GPU test of one row, for the oracle in `mode` against the float64 oracle"""
    out = fwd_checks(name, lambda B: ref_forward(name, B, mode), prec, scale)
    if name in EDGE_CRITICS:
        return out
    for n, cm in CHAIN_CASES:
        for B in CHAIN_BATCHES if n == name else ():
            out.update(chain_checks(name, cm, B, ref_chain(name, cm, B, mode), prec, scale))
    for N in MSE_BATCHES:
        out.update(mse_checks(name, N, ref_mse(name, N, mode), prec, scale))
    for case in PPO_CASES:
        if case[0] == name:
            out.update(ppo_checks(case, ref_ppo(case, mode), prec, scale))
    if name == BC_CASE[0]:
        out.update(bc_checks(ref_bc(mode), prec, scale))
    return out


def ppo_checks(case, got, prec, scale=1.0):
    want = ref_ppo(case)
    cid = case_id(case)
    out = {f"{cid} {k}": v for k, v in scalar_checks("ppo", got[0], want[0], prec, scale, want[3]["ratio_dev"], case[4]).items()}
    out.update(grad_checks(got[1], want[1], prec, f"{cid} actor", scale))
    out.update(grad_checks(got[2], want[2], prec, f"{cid} critic", scale))
    return out


def bc_checks(got, prec, scale=1.0):
    want = ref_bc()
    out = {f"bc {k}": v for k, v in scalar_checks("bc", got[0], want[0], prec, scale).items()}
    out.update(grad_checks(got[1], want[1], prec, "bc", scale))
    return out


@pytest.mark.parametrize("name", ACTOR_NAMES + CRITIC_NAMES)
def test_oracle_float32_agrees_with_float64_to_a_tenth_of_every_bound(name):
    """The fp32 bounds of the GPU tests are for the KERNEL's error: the reference's own rounding (the oracle in float32 against the
    oracle in float64, same inputs) stays under a tenth of each -- forward, chains, log-probs, losses, statistics and every
    gradient tensor, for every (row, batch) the GPU tests use (a critic's PPO cases are checked with their actor's) -- and no
    gradient tensor of the float64 oracle is zero.  A row that comes closer is badly conditioned input: another seed, never
    another bound."""
    checks = all_checks(name, "f32", "fp32", scale=0.1)
    judge(name, "fp32", checks, what=f"{name} oracle float32 vs float64 (a tenth of the bounds)")


MARGIN_BANDS = {"relu": RELU_BAND, "logprob_clamp": CLAMP_BAND, "x0_clamp": CLAMP_BAND, "ratio_clip": RATIO_BAND,
                "value_clip": VCLIP_BAND, "value_max": VCLIP_BAND}


@pytest.mark.parametrize("name", ACTOR_NAMES)
def test_every_decision_of_the_float64_oracle_keeps_its_guard_band(name):
    """A gradient jumps where a ReLU input changes sign, where a clamp that carries a gradient starts to bind (x0 at
    +-denoised_clip_value inside the scored step, a log-prob at -5 or 2) and where the PPO ratio crosses 1 +- clip or the value
    moves past clip_vloss_coef: an input that puts one of them within the kernel's rounding of its kink makes the gradient check
    a coin toss no kernel can win.  On the inputs of this file the float64 oracle keeps every ReLU input (the critic's too)
    RELU_BAND = 1e-5 and every such clamp CLAMP_BAND = 1e-5 from its kink (rows are taken from a pool, judged by the oracle
    alone), |ratio - 1| RATIO_BAND = 5e-3 from the clip range and |V - V_old| VCLIP_BAND = 5e-2 from the value clip (both by
    construction of the old log-probs and values; both sides of each occur).  The advantage-quantile clamp is decided on the
    host from the float32 advantages alone, identically on both sides.  In the sampler and in the scoring pass on its chain,
    every entry of x0 (+-denoised_clip_value), of the final action (+-final_action_clip_value), of eps (+-eps_clip_value) and of
    the noise (+-randn_clip_value) stays CLAMP_BAND from its bound (chain_inputs takes its rows from a pool), and so does the
    step's std from min_sampling_denoising_std / min_logprob_denoising_std, which depends on the schedule alone.  (DDIM's
    clamps of sigma at 1e-10 and of 1 - alpha_prev - sigma^2 at 0 are taken on the schedule's tables, on the host, by both
    sides alike.)"""
    for N in MSE_BATCHES:
        m = ref_mse(name, N)[2]
        assert (m is not None) == relu_row(name)
        if m is not None:
            print(f"{name} mse N={N}: min |ReLU input| {m:.2e}")
            assert m >= RELU_BAND, (N, m)
    cases = [c for c in PPO_CASES if c[0] == name]
    assert cases
    for case in cases:
        m = ref_ppo(case)[3]
        print(f"{case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items() if v is not None))
        assert 0.05 <= m["ratio_dev"] <= 0.2
        for k, band in MARGIN_BANDS.items():
            if m.get(k) is not None:
                assert m[k] >= band, (case_id(case), k, m[k])
        assert m["relu"] is not None or not (relu_row(name) or relu_row(case[1]))
        assert ("value_clip" in m) == ("vclip" in dict(case[5]))
        if case[4] >= 80:
            assert 0.2 <= m["clipped"] <= 0.8, m["clipped"]  # both branches of the surrogate
    if name == BC_CASE[0]:
        m = ref_bc()[2]
        print(f"bc: min |ReLU input| {m['relu']:.2e}, log-prob clamp {m['logprob_clamp']:.2e}")
        assert m["relu"] >= RELU_BAND and m["logprob_clamp"] >= CLAMP_BAND
    for n, cm in CHAIN_CASES:
        for B in CHAIN_BATCHES if n == name else ():
            s, kw = spec(name), CHAIN_KW[cm]
            state, noise = chain_inputs(name, cm, B)
            cfg, base, ft = make_cfg(s, kw), params(s, SEED_BASE, F64), ft_params(s, F64)
            with oracle_mode(), _Decisions() as d, torch.no_grad():  # the sampler, then the scoring pass on the chain as handed over
                chains = O.sample_chain(cfg, s, base, ft, state.double(), noise.double())[1]
                O.chain_logprob(cfg, s, base, ft, state.double(), chains.float().double())
            near = {f"clamp at {b:g}": d.nearest(b) for b in chain_bounds(kw)}
            near["std clip"] = d.nearest(kw.get("min_sampling_denoising_std", 0.1))
            print(f"{name} {cm} B={B}: " + ", ".join(f"{k} {v:.2e}" for k, v in near.items()))
            assert len(near) == (4 if cm == "ddim" else 3) and all(v is not None and v >= CLAMP_BAND for v in near.values()), near


def test_bf16_bounds_from_the_rounded_oracle_are_needed():
    """A row takes its bf16 bounds from the rounded oracle exactly when bf16 operands alone (float64 arithmetic, no kernel) use up
    more than half of one of the usual bounds on one of its checks; every other row keeps the usual bounds.  The rounded
    oracle is float64 arithmetic on the CPU, whose last bits depend on the BLAS at hand and can move a value through a bfloat16
    tie, so "half" is decided with a margin: a row over 0.55 of a bound must be listed, a row under 0.45 of every bound must not
    be, and a row in between (h512_out128, 0.495 of the 3 % on time_embedding.1.bias at M = 1300) may be either -- judge()
    consults the yardstick check by check, and where it is under half a bound the usual bound holds, listed or not."""
    must, may = set(), set()
    for name in ACTOR_NAMES + CRITIC_NAMES:
        checks = all_checks(name, "bf16ops", "bf16")  # (a critic's PPO checks are made, and judged, with its actor's)
        k = max(checks, key=lambda k: checks[k][0] / checks[k][1] if checks[k][1] else float("inf"))
        v, b = checks[k]
        print(f"{name}: bf16 operands alone use at most {v / b:.3f} of a bound ({k}: {v:.3e}, bound {b:.1e})")
        must |= {name} if v > 0.55 * b else set()
        may |= {name} if v > 0.45 * b else set()
    assert must <= BF16_FROM_ROUNDED_ORACLE <= may, (sorted(must - BF16_FROM_ROUNDED_ORACLE), sorted(BF16_FROM_ROUNDED_ORACLE - may))


@pytest.mark.parametrize("name", ACTOR_NAMES + CRITIC_NAMES)
def test_flat_parameter_layout_matches_the_oracle(name):
    """dppo_net_param_count, the state-dict names and the flat order against O.param_shapes, and a packed image of positive size
    in both precisions."""
    from dppo_amd import hip
    s, lib = spec(name), hip.load()
    m = hip_net(name, 1, "fp32", dev="cpu")
    shapes = O.param_shapes(s)
    assert [k for k, _ in m.named_parameters()] == [n for n, _, _ in shapes] == list(m.state_dict())
    assert [tuple(p.shape) for p in m.parameters()] == [sh for _, sh, _ in shapes]
    d = m.net_desc()
    assert (d.in_dim, d.out_dim, d.hidden, d.n_blocks) == (s.in_dim, s.out_dim, s.mlp_dims[0], (len(s.mlp_dims) - 1) // 2)
    total = sum(int(np.prod(sh)) for _, sh, _ in shapes)
    assert lib.dppo_net_param_count(C.byref(d)) == total == m.flat_params().numel()
    flat, off = m.flat_params(), 0
    for p in m.parameters():  # parameters are views of the flat image, in the oracle's order
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        off += p.numel()
    for prec in (hip.PREC_F32, hip.PREC_BF16):
        assert lib.dppo_packed_bytes(C.byref(d), prec, K if s.kind == "actor" else 0) > 0, lib.dppo_last_error()


def _desc(**over):
    from dppo_amd import hip
    kw = dict(kind=0, in_dim=4 + 16 + 8, hidden=256, n_blocks=1, out_dim=4, act=hip.ACT_RELU, time_dim=16, act_flat=4, cond_dim=8,
              cond_hidden=0, cond_out=0, use_layernorm=0, plain=0)
    kw.update(over)
    return hip.NetDesc(**kw)


REFUSED = [  # (what differs from h256_room's descriptor, a piece of check_net()'s message)
    (dict(n_blocks=9), "n_blocks=9 out of [0,8]"), (dict(n_blocks=-1), "n_blocks=-1 out of [0,8]"),
    (dict(out_dim=0, act_flat=0, in_dim=24), "out_dim=0 out of [1,1024]"),
    (dict(out_dim=129, act_flat=129, in_dim=129 + 24), "a denoiser's out_dim = Ta*Da must be <= 128"),
    (dict(time_dim=2, in_dim=4 + 2 + 8), "time_dim=2 must be even and >= 4"), (dict(time_dim=5, in_dim=4 + 5 + 8), "time_dim=5 must be even and >= 4"),
    (dict(cond_dim=1005, in_dim=1025), "in_dim=1025 out of [1,1024]"),
    (dict(kind=1, in_dim=1025, cond_dim=1025, out_dim=1, time_dim=0, act_flat=0), "in_dim=1025 out of [1,1024]"),
    (dict(in_dim=29), "actor in_dim mismatch"), (dict(act_flat=3), "actor out_dim must equal act_flat"),
    (dict(kind=1, in_dim=9, out_dim=1, time_dim=0, act_flat=0), "critic in_dim must equal cond_dim"),
    (dict(cond_hidden=24), "cond_hidden / cond_out must both be set or both 0"),
    (dict(cond_hidden=24, cond_out=257, in_dim=4 + 16 + 257), "cond_mlp dims out of range"),
    (dict(cond_hidden=24, cond_out=8, time_dim=6, in_dim=4 + 6 + 8), "cond_mlp needs Ta*Da + time_dim to be a multiple of 4"),
    (dict(hidden=384, use_layernorm=1), "LayerNorm blocks need hidden in {256, 512, 1024}"),
    (dict(hidden=192), "hidden=192 must be a positive multiple of 128"), (dict(act=2), "activation 2 unsupported"),
]
ACCEPTED = [dict(), dict(n_blocks=0), dict(n_blocks=8), dict(out_dim=128, act_flat=128, in_dim=128 + 24), dict(out_dim=1, act_flat=1, in_dim=25),
            dict(time_dim=4, in_dim=16), dict(cond_dim=1004, in_dim=1024), dict(cond_hidden=24, cond_out=256, in_dim=4 + 16 + 256),
            dict(hidden=384), dict(hidden=1152), dict(hidden=512, use_layernorm=1)]


def test_descriptors_are_refused_by_message_without_a_launch():
    """One refusal (or more) per line of check_net() that tests/test_abi.py does not assert: -1 with the line's message from the
    parameter count, the packed size, the PPO workspace size and the route export (none of which launches), and a good descriptor
    is accepted right after each refusal.  The other side of each limit is accepted."""
    from dppo_amd import hip
    lib = hip.load()
    ok, critic = _desc(cond_dim=32, in_dim=4 + 16 + 32), actor_desc("c256_in32")
    good = lib.dppo_net_param_count(C.byref(ok))
    assert good > 0
    mask = C.c_int(0)
    for over, msg in REFUSED:
        d = _desc(**over)
        for call in (lambda: lib.dppo_net_param_count(C.byref(d)), lambda: lib.dppo_packed_bytes(C.byref(d), hip.PREC_BF16, K),
                     lambda: lib.dppo_ppo_workspace_bytes(C.byref(d) if d.kind == 0 else C.byref(ok), C.byref(critic) if d.kind == 0 else C.byref(d),
                                                          hip.PREC_F32, 64),
                     lambda: lib.dppo_backward_route(C.byref(d), hip.PREC_BF16, 64, KFT, 0, C.byref(mask))):
            assert call() == -1, over
            assert msg in lib.dppo_last_error().decode(), (over, lib.dppo_last_error().decode())
        assert lib.dppo_net_param_count(C.byref(ok)) == good
    for over in ACCEPTED:
        d = _desc(**over)
        assert lib.dppo_net_param_count(C.byref(d)) > 0, (over, lib.dppo_last_error().decode())
        assert lib.dppo_ppo_workspace_bytes(C.byref(d), C.byref(critic), hip.PREC_BF16, 64) > 0, over
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    with pytest.raises(NotImplementedError, match="LayerNorm blocks need a hidden width of 256, 512 or 1024"):  # the Python side of it
        DiffusionMLP(3, 2, 5, time_dim=6, mlp_dims=[384] * 5, residual_style=True, use_layernorm=True)


# ------------------------------------------------------------------ 4. GPU
PRECS = ["fp32", "bf16"]


def ppo_model(aname, cname, kw, prec, mix=1.0):
    from dppo_amd.model.diffusion.diffusion_ppo import PPODiffusion
    from dppo_amd.model.diffusion.eta import EtaFixed
    a = spec(aname)
    kw = dict(kw)
    if kw.get("use_ddim"):
        kw["eta"] = EtaFixed(base_eta=1.0)
    kw.setdefault("gamma_denoising", 0.99)
    kw.setdefault("clip_ploss_coef", 0.01)
    m = PPODiffusion(actor=hip_net(aname, SEED_BASE, prec, dev="cpu"), critic=hip_net(cname, SEED_CRITIC, prec, dev="cpu"),
                     horizon_steps=a.horizon_steps, obs_dim=a.cond_dim, action_dim=a.action_dim, device=DEV, **kw)
    m.actor_ft.load_state_dict(ft_params(a, F32, mix), strict=True)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ACTOR_NAMES + CRITIC_NAMES)
def test_hip_forward(name, prec):
    """DiffusionMLP.forward / CriticObs.forward (dppo_mlp_forward) at B = 1, 17, 130: one row, a ragged tile, two row tiles."""
    m = hip_net(name, SEED_FWD, prec)

    def run(B):
        inp = [v.to(DEV) for v in fwd_inputs(name, B)]
        out = m({"state": inp[0]}) if len(inp) == 1 else m(inp[0], inp[1], {"state": inp[2]})
        return out.cpu().numpy()
    judge(name, prec, fwd_checks(name, run, prec), lambda: fwd_checks(name, lambda B: ref_forward(name, B, "bf16ops"), "bf16"),
          f"{name} forward")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,cm", CHAIN_CASES)
def test_hip_chains_and_logprobs(name, cm, prec):
    """The K-step sampler with recorded noise (DDPM K = 20, Kft = 10 with the x0 and the final-action clamp; DDIM 100 / 5 with the
    eps clamp and min_sampling_denoising_std 0.04) and the chain log-probs of the FLOAT64 ORACLE's OWN chains (every entry: none
    lies in the tail), B = 3 and 17.  Where the sampler refuses the row (SAMPLER_REFUSED) the call raises the library's message
    and the log-probs, which go through the layered forward, are held all the same."""
    from dppo_amd import hip
    m = ppo_model(name, f"std{spec(name).cond_dim}", CHAIN_KW[cm], prec)
    for B in CHAIN_BATCHES:
        state, noise = chain_inputs(name, cm, B)
        cond = {"state": state.to(DEV)}
        if (name, prec) in SAMPLER_REFUSED:
            with pytest.raises(hip.DppoHipError, match=SAMPLER_REFUSED[(name, prec)]):
                m(cond=cond, deterministic=False, return_chain=True, noise=noise.to(DEV))
            chains = traj = None
        else:
            smp = m(cond=cond, deterministic=False, return_chain=True, noise=noise.to(DEV))
            chains, traj = smp.chains.cpu().numpy(), smp.trajectories.cpu().numpy()
        lp = m.get_logprobs(cond, T(ref_chain(name, cm, B)[0]).float().to(DEV)).cpu().numpy()
        judge(name, prec, chain_checks(name, cm, B, (chains, traj, lp), prec),
              lambda: chain_checks(name, cm, B, ref_chain(name, cm, B, "bf16ops"), "bf16"),
              f"{name} {cm} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ACTOR_NAMES)
def test_hip_denoise_mse_and_grads(name, prec):
    """DiffusionModel.p_losses (dppo_denoise_mse_fwd_bwd: the pre-training backward, route flag SIDE with K = 20 one-hot columns)
    at N = 12 and 130: the loss and every gradient tensor."""
    from dppo_amd.model.diffusion.diffusion import DiffusionModel
    s = spec(name)
    net = hip_net(name, SEED_MSE, prec, dev="cpu")
    m = DiffusionModel(network=net, horizon_steps=s.horizon_steps, obs_dim=s.cond_dim, action_dim=s.action_dim, device=DEV,
                       denoising_steps=K)
    for N in MSE_BATCHES:
        x0, state, t, noise = (v.to(DEV) for v in mse_inputs(name, N))
        for p in net.parameters():
            p.grad = None
        loss = m.p_losses(x0, {"state": state}, t, noise=noise)
        loss.backward()
        got = (loss.item(), {k: p.grad.cpu().numpy() for k, p in net.named_parameters()})
        judge(name, prec, mse_checks(name, N, got, prec), lambda: mse_checks(name, N, ref_mse(name, N, "bf16ops"), "bf16"),
              f"{name} denoising loss N={N}")


def run_ppo(case, prec):
    """(statistics, actor gradients, critic gradients) of PPODiffusion.ppo_update on ppo_batch(case)"""
    aname, cname, R, Kft, M, _ = case
    m = ppo_model(aname, cname, ppo_kw(case), prec)
    b = ppo_batch(case)
    d = lambda k, *shape: b[k].reshape(*shape).contiguous().to(DEV)
    st = m.ppo_update(d("state", R, -1), d("chains", R, Kft + 1, -1), d("ret", R), d("oldv", R), d("adv", R), d("oldlp", R, Kft, -1),
                      b["inds"].to(DEV).contiguous(), reward_horizon=b["reward_horizon"]).cpu().numpy().copy()
    ga = {k: g.detach().cpu().numpy().copy() for (k, _), g in zip(m.actor_ft.named_parameters(), m.actor_ft.grad_views())}
    gc = {k: g.detach().cpu().numpy().copy() for (k, _), g in zip(m.critic.named_parameters(), m.critic.grad_views())}
    return st[:5], ga, gc


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", PPO_CASES, ids=case_id)
def test_hip_ppo_update(case, prec):
    """PPODiffusion.ppo_update (dppo_ppo_loss_fwd_bwd) on a rollout buffer of the float64 oracle's own chains: pg_loss, v_loss,
    approx_kl, clipfrac, the mean ratio and every gradient tensor of the actor (pg_loss) and of the critic (v_loss), at the
    (R, Kft, M) of the case -- the route it takes is the one ROUTES pins."""
    checks = ppo_checks(case, run_ppo(case, prec), prec)
    print("{} {}: approx_kl off by {:.2e} (bound {:.2e})".format(case_id(case), prec, *checks[f"{case_id(case)} approx_kl"]))
    judge(case[0], prec, checks, lambda: ppo_checks(case, ref_ppo(case, "bf16ops"), "bf16"), case_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_hip_bc_term(prec):
    """The behaviour-cloning term (dppo_bc_loss_fwd_bwd) on recorded noise: base-policy chains from the sampler, scored by a
    fine-tuned network BC_MIX of the way from the base network, so that every log-prob stays inside the [-5, 2] clamp."""
    name, B, Kft = BC_CASE
    m = ppo_model(name, f"std{spec(name).cond_dim}", BC_KW, prec, mix=BC_MIX)
    state, noise = bc_inputs()
    value, grad = m.bc_loss_and_grad({"state": state.to(DEV)}, noise=noise.to(DEV))
    g, off = {}, 0
    for k, p in m.actor_ft.named_parameters():
        g[k] = grad[off:off + p.numel()].view(p.shape).cpu().numpy()
        off += p.numel()
    judge(name, prec, bc_checks((float(value.item()), g), prec), lambda: bc_checks(ref_bc("bf16ops"), "bf16"), "bc term")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in PPO_CASES if case_id(c) in ("h512_out64-std8-R8-Kft10-M80", "h256_room-std8-R130-Kft10-M1300")],
                         ids=case_id)
def test_hip_precisions_interleaved_in_one_process(case):
    """fp32, then bf16, then fp32 again on one network in one process (h512_out64 merges its forward in bf16 only; h256_room
    takes the in-kernel dW0 in bf16 only): all three meet their bounds and the two fp32 results are the same bits, whatever
    ran in between (per-instantiation launch attributes, cached packed images and workspaces)."""
    runs = [run_ppo(case, prec) for prec in ("fp32", "bf16", "fp32")]
    for prec, got in zip(("fp32", "bf16", "fp32"), runs):
        judge(case[0], prec, ppo_checks(case, got, prec), lambda: ppo_checks(case, ref_ppo(case, "bf16ops"), "bf16"),
              case_id(case) + " interleaved")
    np.testing.assert_array_equal(runs[0][0], runs[2][0])
    for i in (1, 2):
        for k in runs[0][i]:
            np.testing.assert_array_equal(runs[0][i][k], runs[2][i][k], err_msg=k)
