"""Case tables, seeded recipes and a plain-torch restatement shared by make_golden_qsm.py (generator, needs the reference) and
tests/test_qsm.py (no reference needed): QSM's TD critic loss, the twin critic's action gradient g, the actor loss on it, and
one update sequence.

Nothing large is stored in g25_qsm.npz: weights come from ``oracle.dppo_oracle.init_params``, inputs from the seeded numpy
recipes below; the fixture holds what only the reference can say (losses, statistics, g, gradients, stepped weights).  The
restatement at the bottom rebuilds every one of those numbers from the oracle's forwards and ``torch.autograd.grad``: it pins the
fixture without a GPU."""
import numpy as np
import torch

from oracle import dppo_oracle as O

# name -> (obs_dim, Ta, Da, denoising steps K, residual_tyle, q_grad_coeff, actor NetSpec)
_A = lambda od, ta, da, dims, act, td: O.NetSpec("actor", cond_dim=od, mlp_dims=dims, activation=act, residual=True, action_dim=da,
                                                 horizon_steps=ta, time_dim=td)
QSM_NETS = {
    # gym/scratch/hopper-v2/qsm_diffusion_mlp.yaml: one-step chunks, AD = 3 (below one 16-byte store), Q in_dim 14, K = 10
    "scratch": (11, 1, 3, 10, False, 50.0, _A(11, 1, 3, [512, 512, 512], "ReLU", 16)),
    "hopper": (11, 4, 3, 20, False, 10.0, O.named_specs("hopper")[0]),        # Q in_dim 23
    # Q in_dim 171, action columns 59..170; the actor at half the shipped width (the fixture stays below the file-size limit)
    "transport": (59, 8, 14, 20, False, 10.0, _A(59, 8, 14, [512, 512, 512], "Mish", 16)),
    "hopper_res": (11, 4, 3, 20, True, 10.0, O.named_specs("hopper")[0]),     # residual twin: loss_critic only
}
QSM_SIZES = (77, 1000)  # a ragged tile; the shipped batch
CRITIC_CASES = [(net, n) for net in ("scratch", "hopper", "transport") for n in QSM_SIZES] + [("hopper_res", 77)]
ACTOR_CASES = [(net, n) for net in ("scratch", "hopper", "transport") for n in QSM_SIZES]
SEED_Q1, SEED_Q2, SEED_ACTOR, SEED_TARGET = 251, 252, 254, 255
WEIGHT_SCALE = 3.0   # of the critics' seeded weights: outputs and action gradients of O(1)
TARGET_EPS = 0.05    # target = Q + TARGET_EPS * (a seeded draw of the same recipe)
GAMMA, REWARD_SCALE = 0.99, 0.01
SAMPLING_KW = dict(randn_clip_value=3, min_sampling_denoising_std=0.1)
# the recorded update sequence (hopper, N = 77): AdamW(lr, betas (0.9, 0.999), eps 1e-8, weight_decay 0) steps, then Polyak
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU = 1e-3, 1e-4, 0.005


def shapes(net):
    """(obs_dim, Ta, Da, K) of a case's networks."""
    return QSM_NETS[net][:4]


def coeff(net):
    return QSM_NETS[net][5]


def actor_spec(net):
    return QSM_NETS[net][6]


def q_spec(net):
    od, ta, da, _ = shapes(net)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=[256, 256, 256], activation="Mish", residual=QSM_NETS[net][4])


def twin_params(net, eps=0.0):
    """State dict of CriticObsAct: Q1 and Q2 from distinct seeds; eps != 0 adds the target's perturbation."""
    spec, out = q_spec(net), {}
    for i, seed in enumerate((SEED_Q1, SEED_Q2)):
        p, d = O.init_params(spec, seed, WEIGHT_SCALE), O.init_params(spec, SEED_TARGET + 10 * i, WEIGHT_SCALE)
        for k in p:
            out[k.replace("Q1.", f"Q{i + 1}.")] = p[k] + np.float32(eps) * d[k] if eps else p[k]
    return out


def actor_params(net):
    return O.init_params(actor_spec(net), SEED_ACTOR)


def inputs(net, n):
    """The n seeded transitions of case (net, n) and the draws both losses take from outside: obs, next_obs (n, 1, Do), actions,
    next_actions (n, Ta, Da), reward scaled by REWARD_SCALE, terminated in {0, 1}, noise (n, Ta, Da) ~ N(0, 1), t (n,) in [0, K)."""
    od, ta, da, K = shapes(net)
    rs = np.random.RandomState(2500 + 7 * list(QSM_NETS).index(net) + n)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, nxt, act, nact = f(n, 1, od), f(n, 1, od), f(n, ta, da), f(n, ta, da)
    reward = torch.from_numpy((REWARD_SCALE * rs.uniform(0, 4, size=n)).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=n) < 0.3).astype(np.float32))
    noise = torch.from_numpy(rs.randn(n, ta, da).astype(np.float32))
    t = torch.from_numpy(rs.randint(0, K, size=n).astype(np.int64))
    return dict(obs=obs, next_obs=nxt, actions=act, next_actions=nact, reward=reward, terminated=terminated, noise=noise, t=t)


# ---- the restatement: the two QSM losses and g in plain torch on the oracle's forwards ---------------------------------------
def twin_forward(params, net, obs, act):
    """(q1, q2), each (n,), of a CriticObsAct state dict on cat[obs, action] (reference critic.py:96-113)."""
    spec = q_spec(net)
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    trunk = lambda i: {k.replace(f"Q{i}.", "Q1."): v for k, v in params.items() if k.startswith(f"Q{i}.")}
    return tuple(O.critic_forward(trunk(i), spec, x).reshape(-1) for i in (1, 2))


def critic_loss(q_params, target_params, net, b):
    """diffusion_qsm.py:65-95 with ``forward`` replaced by the recipe's next_actions -> (loss, mean q1, mean y)."""
    q1, q2 = twin_forward(q_params, net, b["obs"], b["actions"])
    with torch.no_grad():
        nq = torch.min(*twin_forward(target_params, net, b["next_obs"], b["next_actions"]))
    y = b["reward"].view(-1) + GAMMA * nq.view(-1) * (1 - b["terminated"]).view(-1)
    return torch.mean((q1 - y) ** 2) + torch.mean((q2 - y) ** 2), q1.detach().double().mean(), y.double().mean()


def action_gradient(q_params, net, b):
    """(x_t, g): diffusion_qsm.py:41-55, g = mean(dQ1/da, dQ2/da) at (obs, x_t), (n, Ta, Da)."""
    x = O.q_sample(shapes(net)[3], b["actions"], b["t"], b["noise"]).detach().requires_grad_(True)
    q1, q2 = twin_forward(q_params, net, b["obs"], x)
    g1 = torch.autograd.grad(q1.sum(), x, retain_graph=True)[0]
    g2 = torch.autograd.grad(q2.sum(), x)[0]
    return x.detach(), torch.stack((g1, g2), 0).mean(0).detach()


def actor_loss(actor_p, q_params, net, b):
    """diffusion_qsm.py:57-63: mse(-eps_theta(x_t, t, obs), coeff * g)."""
    x, g = action_gradient(q_params, net, b)
    pred = O.actor_forward(actor_p, actor_spec(net), x, b["t"], b["obs"])
    return torch.nn.functional.mse_loss(-pred, coeff(net) * g), g


def leaf(params):
    return {k: v.clone().requires_grad_(True) for k, v in params.items()}


def restate_sequence(net, b):
    """One update on ``b`` in the reference agent's order (:246-275): critic loss and AdamW step, actor loss with the UPDATED
    critic and its step, Polyak.  Returns what make_golden_qsm.update_sequence records."""
    q, tq, a = leaf(twin_params(net)), twin_params(net, TARGET_EPS), leaf(actor_params(net))
    opt_c = torch.optim.AdamW(list(q.values()), lr=SEQ_LR, weight_decay=0)
    opt_a = torch.optim.AdamW(list(a.values()), lr=SEQ_ACTOR_LR, weight_decay=0)
    lc, _, _ = critic_loss(q, tq, net, b)
    lc.backward()
    gq = {k: v.grad.clone() for k, v in q.items()}
    opt_c.step()
    q2 = {k: v.detach() for k, v in q.items()}
    la, _ = actor_loss(a, q2, net, b)
    la.backward()
    ga = {k: v.grad.clone() for k, v in a.items()}
    opt_a.step()
    t2 = {k: tq[k] * (1.0 - SEQ_TAU) + q2[k] * SEQ_TAU for k in tq}
    return dict(c_loss=lc.item(), a_loss=la.item(), gq=gq, ga=ga, q=q2, actor={k: v.detach() for k, v in a.items()}, target=t2)
