"""Case table, seeded recipes and a plain-torch restatement of the reference's IBRL model (model/rl/gaussian_ibrl.py: ``forward``
:149-205, ``loss_critic`` :69-113) with its dropout actor (model/common/mlp.py:59-60, model/common/mlp_gaussian.py:323-329,
model/common/gaussian.py:67-120), shared by tests/test_ibrl.py, tests/test_ibrl_dropout.py and make_golden_ibrl.py.

Weights and inputs come from the seeded numpy recipes below and are never stored.  The restatement is written the way the reference
writes it and takes a dtype: float64 fed the same fp32 values is the yardstick of the GPU tests.  Every draw is an input: the two
actors' Gaussian noise, their dropout masks (uint8 [L][n][H], 1 = keep, applied as ``x * (mask / (1 - p))``, torch's own product),
the uniform ``u`` of the soft choice and the pair of members.  ``bf16_linears`` / ``relu_gates`` are make_golden_dql_cases.py's
contexts (LayerNorm, dropout and the heads stay in fp32 under ``bf16_linears``: it rounds ``F.linear``'s operands only).

Constructed rows (a case with n >= 3 carries both; tiny_1 has one row and carries neither):
  * TIE_ROW: both proposals are the same action, so the two Q are equal and the strict ``>`` must take RL.  With dropout the row's
    masks drop the whole last hidden layer in both actors and both draws are 0: the action is tanh(out bias), which the actors share;
    without dropout (nodrop) the three actors are equal, as they are right after construction, and both draws are 0.
  * OVF_ROW (``forward`` only): observation coordinate 0 is FLAG.  LayerNorm makes layer 0's output of that row the same spike
    whatever else the row holds; every member's out layer gets a rank-one correction along that row's last hidden features, made
    orthogonal to the other rows' mean features, which lifts the row's Q by OVF_LIFT and the other rows' by zero on average.  At beta
    = 10 both exp(beta q) overflow fp32 there.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dppo_oracle as O
from tests.golden.make_golden_dql_cases import RELU_TIE, bf16_linears, relu_gates  # noqa: F401  (re-exported)
from tests.golden.make_golden_sac_cases import Q_CEIL  # noqa: F401  (the guard band's unit)

# case -> (obs_dim, Ta, Da, actor widths, actor activation, dropout p, critic widths, critic activation, E)
IBRL_NETS = {
    "tiny": (11, 1, 3, [64, 64], "ReLU", 0.5, [64, 64], "ReLU", 3),
    "chunk": (23, 4, 7, [128, 128, 128], "Mish", 0.25, [128, 128, 128], "Mish", 5),  # 1 / (1 - p) is no power of two
    "nodrop": (17, 1, 6, [256, 256, 256], "ReLU", 0.0, [256, 256, 256], "ReLU", 2),  # halfcheetah's form: the null-struct path
    "can": (23, 1, 7, [1024, 1024, 1024], "ReLU", 0.5, [1024, 1024, 1024], "ReLU", 5),  # robomimic/finetune/can/ibrl_mlp.yaml
}
CASES = [("tiny", 1), ("tiny", 77), ("chunk", 130), ("nodrop", 64), ("can", 256)]
PAIRS = {"tiny": (2, 0), "chunk": (1, 4), "nodrop": (1, 0), "can": (3, 1)}  # tiny's is reversed: the pair's order matters
FIXED_STD, BC_STD, RANDN_CLIP = 0.1, 1e-4, 3.0
GAMMA, BETA = 0.99, 10.0
SEED_ACTOR, SEED_Q, SEED_TARGET = 3101, 3131, 3161
Q_SCALE, TARGET_EPS, ACTOR_EPS = 3.0, 0.05, 0.25
TIE_ROW, OVF_ROW, FLAG, OVF_LIFT = 2, 1, 1000.0, 16.0
CLIP_BAND, U_BAND = 2e-2, 1e-3
EXP_OVERFLOW = 88.7229  # exp(x) is inf in fp32 from 88.72284 on
U_SEEDS = {"tiny": 3400, "chunk": 3400, "nodrop": 3400, "can": 3401}  # chosen so that every |u - p_bc| keeps U_BAND


def shapes(case):
    return IBRL_NETS[case][:3]


def n_critics(case):
    return IBRL_NETS[case][8]


def dropout(case):
    return IBRL_NETS[case][5]


def pair_of(case):
    return PAIRS[case]


def actor_spec(case):
    od, ta, da, dims, act = IBRL_NETS[case][:5]
    return O.NetSpec("gaussian", cond_dim=od, mlp_dims=list(dims), activation=act, residual=False, action_dim=da, horizon_steps=ta)


def q_spec(case):
    od, ta, da = shapes(case)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=list(IBRL_NETS[case][6]), activation=IBRL_NETS[case][7], residual=False,
                     use_layernorm=True)


def special_rows(n):
    """(tie row or None, overflow row or None)."""
    return (TIE_ROW, OVF_ROW) if n >= 3 else (None, None)


@functools.lru_cache(maxsize=None)
def _actor_base(case):
    k = list(IBRL_NETS).index(case)
    return O.init_params(actor_spec(case), SEED_ACTOR + k), O.init_params(actor_spec(case), SEED_ACTOR + 10 + k)


def actor_params(case, which):
    """Trunk state dict (mlp_mean.moduleList.{i}.linear_1.*) of ``which`` in {"bc", "rl", "target"}: the imitation policy, and two
    perturbations of it that keep its out bias (TIE_ROW); without dropout all three are the imitation policy."""
    p, d = _actor_base(case)
    eps = 0.0 if dropout(case) == 0 else {"bc": 0.0, "rl": ACTOR_EPS, "target": -ACTOR_EPS}[which]
    last = f"mlp_mean.moduleList.{len(IBRL_NETS[case][3])}.linear_1.bias"
    return {k: (p[k] + np.float32(eps) * d[k] if eps and k != last else p[k].clone()) for k in p}


def actor_state_dict(case, which, std_min=0.01, std_max=1.0):
    """The whole Gaussian_MLP state dict, in the reference's order."""
    sd = dict(actor_params(case, which))
    sd["logvar_min"] = torch.log(torch.tensor(std_min ** 2))
    sd["logvar_max"] = torch.log(torch.tensor(std_max ** 2))
    return sd


def _base_member(case, e, eps):
    spec, k = q_spec(case), 100 * list(IBRL_NETS).index(case) + e
    p, d = O.init_params(spec, SEED_Q + k, Q_SCALE), O.init_params(spec, SEED_TARGET + k, Q_SCALE)
    if eps:
        p = {key: p[key] + np.float32(eps) * d[key] for key in p}
    return p


def _hidden_features(p, case, x):
    """The last hidden layer's activations of one member, (n, H)."""
    spec = q_spec(case)
    fn = O._ACT[spec.activation]
    for i in range(len(spec.mlp_dims)):
        pre = f"Q1.moduleList.{i}"
        x = F.linear(x, p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])
        x = fn(F.layer_norm(x, x.shape[-1:], p[f"{pre}.norm_1.weight"], p[f"{pre}.norm_1.bias"], 1e-5))
    return x


@functools.lru_cache(maxsize=None)
def _members(case, eps):
    """All E members with OVF_ROW's correction (module docstring): computed once in float64 on the largest n of the case, rounded to
    fp32 once."""
    n = max(k for c, k in CASES if c == case)
    od, ta, da = shapes(case)
    obs = torch.cat([forward_inputs(case, n)["obs"].reshape(n, -1), torch.zeros(n, ta * da)], dim=-1).double()
    out = []
    for e in range(n_critics(case)):
        p = _base_member(case, e, eps)
        with torch.no_grad():
            phi = _hidden_features({k: v.double() for k, v in p.items()}, case, obs)
        star, rest = phi[OVF_ROW], torch.cat([phi[:OVF_ROW], phi[OVF_ROW + 1:]]).mean(dim=0)
        d = star - (star @ rest) / (rest @ rest) * rest
        key = f"Q1.moduleList.{len(IBRL_NETS[case][6])}.linear_1.weight"
        p[key] = (p[key].double() + OVF_LIFT * d / (d @ star)).float().reshape(p[key].shape)
        out.append(p)
    return out


def member_params(case, e, eps=0.0):
    """State dict of member e: CriticObsAct(use_layernorm=True, double_q=False), in the reference's order.  eps != 0: the target's."""
    return {k: v.clone() for k, v in _members(case, eps)[e].items()}


def _draws(rs, case, n, tie):
    """Gaussian noise (n, Ta, Da) kept CLIP_BAND away from the clip on either side, some of it beyond, and a dropout mask
    (L, n, H); on the tie row the draw is 0 and the last hidden layer is dropped whole."""
    od, ta, da, dims = IBRL_NETS[case][:4]
    z = (1.5 * rs.standard_normal(size=(n, ta, da))).astype(np.float32)
    near = np.abs(np.abs(z) - RANDN_CLIP) < 2 * CLIP_BAND
    z = np.where(near, z * np.float32(0.9), z)
    mask = (rs.uniform(size=(len(dims), n, dims[0])) >= dropout(case)).astype(np.uint8)
    if tie is not None:
        z[tie] = 0
        if dropout(case) > 0:
            mask[-1, tie] = 0
    return torch.from_numpy(z), torch.from_numpy(mask)


@functools.lru_cache(maxsize=None)
def _inputs(case, n):
    od, ta, da = shapes(case)
    rs = np.random.RandomState(3200 + 17 * list(IBRL_NETS).index(case) + n)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, act, nxt = f(n, 1, od), f(n, ta, da), f(n, 1, od)
    reward = torch.from_numpy(rs.uniform(0, 4, size=n).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=n) < 0.3).astype(np.float32))
    tie, _ = special_rows(n)
    noise_bc, mask_bc = _draws(rs, case, n, tie)
    noise_rl, mask_rl = _draws(rs, case, n, tie)
    return dict(obs=obs, actions=act, next_obs=nxt, reward=reward, terminated=terminated, noise_bc=noise_bc, noise_rl=noise_rl,
                mask_bc=mask_bc, mask_rl=mask_rl)


def inputs(case, n):
    """The n seeded transitions of a case and the draws of ``loss_critic``'s two samples at next_obs."""
    return dict(_inputs(case, n))


@functools.lru_cache(maxsize=None)
def _forward_inputs(case, n):
    od, ta, da = shapes(case)
    rs = np.random.RandomState(3300 + 17 * list(IBRL_NETS).index(case) + n)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(n, 1, od)).astype(np.float32))
    tie, ovf = special_rows(n)
    if ovf is not None:
        obs[ovf, 0, 0] = FLAG
    noise_bc, mask_bc = _draws(rs, case, n, tie)
    noise_rl, mask_rl = _draws(rs, case, n, tie)
    u = torch.from_numpy(np.random.RandomState(U_SEEDS[case] + n).uniform(size=n).astype(np.float32))
    return dict(obs=obs, noise_bc=noise_bc, noise_rl=noise_rl, mask_bc=mask_bc, mask_rl=mask_rl, u=u)


def forward_inputs(case, n):
    """The n observations ``forward`` acts on and its draws."""
    return dict(_forward_inputs(case, n))


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def leaf(params, dtype=torch.float32):
    return {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def actor_mean(p, case, obs, mask=None):
    """Gaussian_MLP.forward's mean (n, Ta*Da): the plain MLP with nn.Dropout behind every hidden Linear, in front of the activation,
    then tanh.  ``mask`` None: eval(), or p = 0."""
    spec, pd = actor_spec(case), dropout(case)
    fn = F.mish if spec.activation == "Mish" else O._ACT[spec.activation]  # nn.Mish's own kernel: the chosen actions are held bit for bit
    x = obs.reshape(len(obs), -1)
    L = len(spec.mlp_dims)
    for i in range(L):
        x = F.linear(x, p[f"mlp_mean.moduleList.{i}.linear_1.weight"], p[f"mlp_mean.moduleList.{i}.linear_1.bias"])
        if mask is not None and pd > 0:
            x = x * (mask[i].to(x.dtype) / (1 - pd))
        x = fn(x)
    x = F.linear(x, p[f"mlp_mean.moduleList.{L}.linear_1.weight"], p[f"mlp_mean.moduleList.{L}.linear_1.bias"])
    return torch.tanh(x)


def sample(p, case, obs, mask, noise, std):
    """GaussianModel.forward (:85-120) without the sample's tanh: loc + draw * scale, clamped to loc -+ clip * scale."""
    loc = actor_mean(p, case, obs, mask)
    scale = torch.ones_like(loc) * std
    a = loc + noise.reshape(loc.shape).to(loc.dtype) * scale
    return torch.clamp(a, loc - RANDN_CLIP * scale, loc + RANDN_CLIP * scale), loc


def q_forward(p, case, obs, act):
    """One member's Q (n,): CriticObsAct.forward with double_q=False on cat[obs, action]."""
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    return O.critic_forward(p, q_spec(case), x).reshape(-1)


def forward(case, b, pair, soft, deterministic=False, beta=BETA, dtype=torch.float32, members=None):
    """gaussian_ibrl.py:149-205 with its draws taken from ``b``.  The soft choice is written as the library documents it: BC iff
    u < 1 / (1 + exp(w_rl - w_bc)), the greedy rule where that difference is NaN.  Returns a_bc, a_rl, q_bc, q_rl, took_bc, action,
    and for the soft choice p_bc and the rows where both weights overflow fp32.  ``members``: E dicts in place of the recipe's."""
    with torch.no_grad():
        obs = b["obs"].to(dtype)
        bc, rl = cast(actor_params(case, "bc"), dtype), cast(actor_params(case, "rl"), dtype)
        a_bc, _ = sample(bc, case, obs, b["mask_bc"], b["noise_bc"], BC_STD)
        a_rl, _ = sample(rl, case, obs, b["mask_rl"], b["noise_rl"], BC_STD if deterministic else FIXED_STD)
        m1, m2 = (cast(members[e] if members is not None else member_params(case, e), dtype) for e in pair)
        q_bc = torch.min(q_forward(m1, case, obs, a_bc), q_forward(m2, case, obs, a_bc))
        q_rl = torch.min(q_forward(m1, case, obs, a_rl), q_forward(m2, case, obs, a_rl))
        took = q_bc > q_rl
        res = dict(a_bc=a_bc, a_rl=a_rl, q_bc=q_bc, q_rl=q_rl)
        if soft and not deterministic:
            d = torch.exp(q_rl * beta) - torch.exp(q_bc * beta)
            p_bc = 1 / (1 + torch.exp(d))
            # where both weights overflow FP32 the difference is NaN there; the rule is stated on q so that float64 follows it too
            both = (q_bc * beta > EXP_OVERFLOW) & (q_rl * beta > EXP_OVERFLOW)
            took = torch.where(both | torch.isnan(d), took, b["u"].to(dtype) < p_bc)
            res.update(p_bc=p_bc, nan_rows=both | torch.isnan(d))
        res.update(took_bc=took, action=torch.where(took[:, None], a_bc, a_rl))
    return res


def next_actions(case, b, dtype=torch.float32):
    """loss_critic's two samples at next_obs: bc_policy "deterministic" (sigma 1e-4, drawn all the same), target_actor stochastic."""
    with torch.no_grad():
        nxt = b["next_obs"].to(dtype)
        a_bc, _ = sample(cast(actor_params(case, "bc"), dtype), case, nxt, b["mask_bc"], b["noise_bc"], BC_STD)
        a_rl, _ = sample(cast(actor_params(case, "target"), dtype), case, nxt, b["mask_rl"], b["noise_rl"], FIXED_STD)
    return a_bc, a_rl


def loss_critic(members, targets, case, b, pair, gamma=GAMMA, dtype=torch.float32):
    """gaussian_ibrl.py:69-113 with the pair and the draws given.  ``members``: E dicts of leaf tensors; ``targets``: E plain dicts.
    Returns loss, stats {loss, mean q, mean y}, q (E, n), mb, mr, y (n,), bc_share and grads (one list per member, in its dict's
    order)."""
    a_bc, a_rl = next_actions(case, b, dtype)
    nxt, rewards, terminated = b["next_obs"].to(dtype), b["reward"].to(dtype), b["terminated"].to(dtype)
    with torch.no_grad():
        t1, t2 = (cast(targets[e], dtype) for e in pair)
        mb = torch.min(q_forward(t1, case, nxt, a_bc), q_forward(t2, case, nxt, a_bc))
        mr = torch.min(q_forward(t1, case, nxt, a_rl), q_forward(t2, case, nxt, a_rl))
        next_q = torch.where(mb > mr, mb, mr)
        target_q = rewards + gamma * (1 - terminated) * next_q
    current_q = torch.stack([q_forward(p, case, b["obs"].to(dtype), b["actions"].to(dtype)) for p in members])
    loss = torch.mean((current_q - target_q[None]) ** 2)
    flat = [t for p in members for t in p.values()]
    grads = iter(torch.autograd.grad(loss, flat))
    return dict(loss=loss.detach(), stats=[float(loss.detach()), float(current_q.detach().mean()), float(target_q.mean())],
                q=current_q.detach(), mb=mb, mr=mr, y=target_q, bc_share=float((mb > mr).double().mean()), a_bc=a_bc, a_rl=a_rl,
                grads=[[next(grads) for _ in p] for p in members])
