"""Case table, seeded recipes and a plain-torch restatement for the LayerNorm Q trunks of the reference's RLPD critics
(model/common/mlp.py:46-74 with use_layernorm; model/rl/gaussian_rlpd.py:64-103), shared by tests/test_rlpd.py.

Weights and inputs come from the seeded numpy recipes below.  The restatement is written the way the reference writes it and takes
a dtype: float64 fed the same fp32 values is the yardstick of the GPU tests.  It reuses the oracle's ``_plain_mlp(...,
use_ln=True)`` and ``init_params``, which know ``norm_1`` and eps 1e-5; ``bf16_linears`` / ``relu_gates`` are
make_golden_dql_cases.py's contexts (LayerNorm stays in fp32 under ``bf16_linears``: it rounds ``F.linear``'s operands only)."""
import numpy as np
import torch

from oracle import dppo_oracle as O
from tests.golden.make_golden_dql_cases import RELU_TIE, bf16_linears, relu_gates  # noqa: F401  (re-exported)
from tests.golden.make_golden_sac_cases import Q_CEIL  # noqa: F401  (the guard band's unit)

# case -> (obs_dim, Ta, Da, critic widths, activation, E)
RLPD_NETS = {
    "tiny": (11, 1, 3, [64, 64], "ReLU", 3),            # AF below one 16-byte store; H = 64, the narrowest LayerNorm row
    "chunk": (22, 4, 7, [128, 128, 128], "Mish", 5),    # AF = 28; three hidden layers
    "cheetah": (17, 1, 6, [256, 256], "ReLU", 10),      # gym/scratch/halfcheetah-v2/rlpd_mlp.yaml
    # tiny with member 1's layer 0 flattened (weight 0, bias 0.5): every row's pre-LayerNorm vector is constant, the variance is 0,
    # rstd = 1 / sqrt(eps), xhat = 0, z = beta.  A one-pass variance (E[x^2] - E[x]^2 of 0.25 in fp32) does not give 0 here.
    "tiny_flat": (11, 1, 3, [64, 64], "ReLU", 3),
}
SIZES = (1, 77, 256)
CASES = [(c, n) for c in ("tiny", "chunk", "cheetah") for n in SIZES] + [("tiny_flat", 77)]
FLAT_MEMBER, FLAT_BIAS = 1, 0.5
SEED_Q, SEED_TARGET = 2801, 2851
Q_SCALE, TARGET_EPS = 3.0, 0.05  # as make_golden_qsm_cases.py: outputs of O(1)
VAR_FLOOR = 1e-3                 # outside tiny_flat every row's pre-LayerNorm variance exceeds this: eps 1e-5 decides nothing
LN_EPS = 1e-5
ALPHA, GAMMA = 0.7, 0.99
NO_BACKUP = ("chunk", 77)        # backup_entropy is on everywhere but here


def shapes(case):
    """(obs_dim, Ta, Da) of a case."""
    return RLPD_NETS[case][:3]


def n_critics(case):
    return RLPD_NETS[case][5]


def q_spec(case):
    od, ta, da, dims, act, _ = RLPD_NETS[case]
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=list(dims), activation=act, residual=False, use_layernorm=True)


def member_params(case, e, eps=0.0):
    """State dict of member e: CriticObsAct(use_layernorm=True, double_q=False), in the reference's order (Q1.moduleList.{i}.linear_1
    / norm_1).  eps != 0 adds the target's perturbation."""
    base = case.split("_")[0]  # tiny_flat shares tiny's weights
    spec, k = q_spec(case), 100 * list(RLPD_NETS).index(base) + e
    p, d = O.init_params(spec, SEED_Q + k, Q_SCALE), O.init_params(spec, SEED_TARGET + k, Q_SCALE)
    if eps:
        p = {key: p[key] + np.float32(eps) * d[key] for key in p}
    if case == "tiny_flat" and e == FLAT_MEMBER:
        p["Q1.moduleList.0.linear_1.weight"] = torch.zeros_like(p["Q1.moduleList.0.linear_1.weight"])
        p["Q1.moduleList.0.linear_1.bias"] = torch.full_like(p["Q1.moduleList.0.linear_1.bias"], FLAT_BIAS)
    return p


def inputs(case, n):
    """The n seeded transitions of a case and what the critic loss takes from outside: the policy's sample at next_obs and its
    log-probability (a tanh-squashed action in (-1, 1), a log-probability of a few nats)."""
    od, ta, da = shapes(case)
    rs = np.random.RandomState(2900 + 13 * list(RLPD_NETS).index(case) + n)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, act, nxt = f(n, 1, od), f(n, ta, da), f(n, 1, od)
    reward = torch.from_numpy(rs.uniform(0, 4, size=n).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=n) < 0.3).astype(np.float32))
    next_actions = f(n, ta, da)
    next_logp = torch.from_numpy(rs.uniform(-3, 1, size=n).astype(np.float32))
    return dict(obs=obs, actions=act, next_obs=nxt, reward=reward, terminated=terminated, next_actions=next_actions,
                next_logp=next_logp)


def pair_of(case, n):
    """The pair of target members of a case: (0, 1), a reversed non-adjacent one, one that ends on the last member; tiny_flat's
    holds the flattened member, reversed."""
    if case == "tiny_flat":
        return (FLAT_MEMBER, 0)
    return {1: (0, 1), 77: (2, 0), 256: (1, n_critics(case) - 1)}[n]


def backup_entropy(case, n):
    return (case, n) != NO_BACKUP


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def q_forward(p, case, obs, act):
    """One member's Q (n,): critic.py's CriticObsAct.forward with double_q=False on cat[obs, action]."""
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    return O.critic_forward(p, q_spec(case), x).reshape(-1)


def pre_ln_variances(p, case, obs, act):
    """The biased variance of every row entering every LayerNorm of one member, [layer][n]: what the guard band is asserted on."""
    spec = q_spec(case)
    fn = O._ACT[spec.activation]
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    out = []
    for i in range(len(spec.mlp_dims)):
        pre = f"Q1.moduleList.{i}"
        x = torch.nn.functional.linear(x, p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])
        out.append(x.var(dim=-1, unbiased=False))
        x = fn(torch.nn.functional.layer_norm(x, x.shape[-1:], p[f"{pre}.norm_1.weight"], p[f"{pre}.norm_1.bias"], LN_EPS))
    return out


def leaf(params, dtype=torch.float32):
    return {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}


def loss_critic(members, targets, case, b, pair, backup=True, alpha=ALPHA, gamma=GAMMA, dtype=torch.float32):
    """gaussian_rlpd.py:64-103 with the policy's sample and its log-probability taken from ``b`` and the pair given.  ``members``:
    E dicts of leaf tensors; ``targets``: E plain dicts.  Returns loss, stats {loss, mean q, mean y}, q (E, n), tq (2, n), y (n) and
    grads (one list per member, in its dict's order)."""
    b = {k: v.to(dtype) for k, v in b.items()}
    rewards, terminated = b["reward"], b["terminated"]
    with torch.no_grad():
        next_q1 = q_forward(cast(targets[pair[0]], dtype), case, b["next_obs"], b["next_actions"])
        next_q2 = q_forward(cast(targets[pair[1]], dtype), case, b["next_obs"], b["next_actions"])
        next_q = torch.min(next_q1, next_q2)
        target_q = rewards + gamma * (1 - terminated) * next_q
        if backup:
            target_q = target_q + gamma * (1 - terminated) * alpha * (-b["next_logp"])
    current_q = torch.stack([q_forward(p, case, b["obs"], b["actions"]) for p in members])
    loss = torch.mean((current_q - target_q[None]) ** 2)
    flat = [t for p in members for t in p.values()]
    grads = iter(torch.autograd.grad(loss, flat))
    return dict(loss=loss.detach(), stats=[float(loss.detach()), float(current_q.detach().mean()), float(target_q.mean())], q=current_q.detach(),
                tq=torch.stack([next_q1, next_q2]), y=target_q, grads=[[next(grads) for _ in p] for p in members])
