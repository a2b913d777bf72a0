"""Case table and plain-torch restatement of RLPD's actor loss through the mean of the ensemble's Q (reference
model/rl/gaussian_rlpd.py:100-112), shared by make_golden_rlpd.py (generator, needs the reference) and tests/test_rlpd_actor.py
(no reference needed).

Everything but one case is borrowed: the cases, the members and the observations are make_golden_rlpd_cases.py's (``K``), the
actor, its draws and the tanh-Gaussian sample are make_golden_sac_cases.py's (``S``): the shapes of tiny, chunk and cheetah agree
between the two tables.  The restatement is written the way the reference writes it -- ``S.sample``, the stacked ``q_forward``,
``.mean(0)``, ``-(q + alpha (-logp)).mean()`` -- and takes a dtype: float32 reproduces the g28 fixture, float64 fed the same fp32
values is the yardstick of the GPU tests.  It works under ``K.relu_gates()`` and ``K.bf16_linears()``.

``wide`` is the one case added here: E = 16 members of [1024, 1024] at N = 3, the top of the range the library accepts (K = E * hidden =
16384 in the chains' tail), with a [64, 64] actor.  No fixture holds it: the reference's own value is not needed where the float64
restatement is the yardstick."""
import math

import numpy as np
import torch

from oracle import dppo_oracle as O
from tests.golden import make_golden_rlpd_cases as K
from tests.golden import make_golden_sac_cases as S

WIDE = ("wide", 3)
WIDE_NET = (11, 1, 3, [1024, 1024], "ReLU", 16)
WIDE_ACTOR_DIMS = [64, 64]
SEED_WIDE_Q, SEED_WIDE_ACTOR, SEED_WIDE_INPUTS = 3101, 3151, 3191
CASES = list(K.CASES)
ALL_CASES = CASES + [WIDE]
ALPHA, RANDN_CLIP = K.ALPHA, S.RANDN_CLIP
# the recorded update sequence (cheetah, N = 77): critic_num_update AdamW critic steps with Polyak, one actor, one temperature step
SEQ_CASE, SEQ_N, SEQ_CRITIC_UPDATES = "cheetah", 77, 2
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU, SEQ_LOG_ALPHA, SEQ_WEIGHT_DECAY = 1e-3, 3e-4, 0.005, math.log(K.ALPHA), 0.0


def net_of(case):
    """(obs_dim, Ta, Da, critic widths, activation, E)."""
    return WIDE_NET if case == "wide" else K.RLPD_NETS[case]


def n_critics(case):
    return net_of(case)[5]


def sac_case(case):
    """The case of make_golden_sac_cases.py whose ACTOR architecture this case has (``wide``: tiny's [64, 64] ReLU on 11 -> 3)."""
    return "tiny" if case == "wide" else case.split("_")[0]


def q_spec(case):
    od, ta, da, dims, act, _ = net_of(case)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=list(dims), activation=act, residual=False, use_layernorm=True)


def member_params(case, e):
    if case != "wide":
        return K.member_params(case, e)
    return O.init_params(q_spec(case), SEED_WIDE_Q + e, K.Q_SCALE)


def actor_params(case):
    """State dict of Gaussian_MLP(fixed_std=None, tanh_output=False): ``S.actor_params`` of the base case; ``wide`` repeats its
    recipe on a seed of its own."""
    if case != "wide":
        return S.actor_params(sac_case(case))
    od, ta, da = WIDE_NET[:3]
    rs = np.random.RandomState(SEED_WIDE_ACTOR)
    lmin, lmax = S.logvar_bounds()
    p = {"logvar_min": lmin, "logvar_max": lmax}

    def lin(name, i, o):
        b = 1.0 / math.sqrt(i)
        p[f"{name}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(o, i)).astype(np.float32))
        p[f"{name}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(o,)).astype(np.float32))
    widths = [od] + WIDE_ACTOR_DIMS
    for i in range(len(widths) - 1):
        lin(f"mlp_base.moduleList.{i}.linear_1", widths[i], widths[i + 1])
    lin("mlp_mean.moduleList.0.linear_1", widths[-1], ta * da)
    lin("mlp_logvar.moduleList.0.linear_1", widths[-1], ta * da)
    return p


def inputs(case, n):
    """dict(obs (n, 1, Do), noise (n, Ta, Da)): ``K.inputs``' observations and ``S.inputs``' actor draws; ``wide`` draws its own
    (uniform observations, N(0, 1) draws kept inside NOISE_CAP like S's)."""
    if case != "wide":
        return dict(obs=K.inputs(case, n)["obs"], noise=S.inputs(sac_case(case), n)["noise"])
    od, ta, da = WIDE_NET[:3]
    rs = np.random.RandomState(SEED_WIDE_INPUTS + n)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(n, 1, od)).astype(np.float32))
    z = np.clip(rs.randn(n, ta, da), -S.NOISE_CAP, S.NOISE_CAP)
    return dict(obs=obs, noise=torch.from_numpy(z.astype(np.float32)))


def q_forward(p, case, obs, act):
    """One member's Q (n,): ``K.q_forward`` on this table's spec."""
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    return O.critic_forward(p, q_spec(case), x).reshape(-1)


def pre_ln_variances(p, case, obs, act):
    """``K.pre_ln_variances`` on this table's spec: the biased variance of every row entering every LayerNorm, [layer][n]."""
    spec = q_spec(case)
    fn = O._ACT[spec.activation]
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    out = []
    for i in range(len(spec.mlp_dims)):
        pre = f"Q1.moduleList.{i}"
        x = torch.nn.functional.linear(x, p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])
        out.append(x.var(dim=-1, unbiased=False))
        x = fn(torch.nn.functional.layer_norm(x, x.shape[-1:], p[f"{pre}.norm_1.weight"], p[f"{pre}.norm_1.bias"], K.LN_EPS))
    return out


def loss_actor(actor_p, members, case, obs, noise, alpha=ALPHA, dtype=torch.float32):
    """gaussian_rlpd.py:100-112 with rsample's draw replaced by ``noise``.  ``actor_p``: leaf tensors of ``dtype``; ``members``: E
    plain dicts.  Returns dict(loss, stats {loss, mean of the members' mean q, mean logp, mean sigma}, d_a = d mean(-q_mean) / d a,
    grads (one per entry of actor_p that takes a gradient, in its order), u, a, logp, q (E, n), g_members (E, n, AF) = d q_e / d a,
    sample)."""
    obs = obs.to(dtype)
    s = S.sample(actor_p, sac_case(case), obs, noise)
    qs = torch.stack([q_forward(K.cast(p, dtype), case, obs, s["a"]) for p in members])
    current_q = qs.mean(dim=0) + alpha * (-s["logp"])
    loss = -torch.mean(current_q)
    d_a = torch.autograd.grad((-qs.mean(dim=0)).mean(), s["a"], retain_graph=True)[0]
    g_members = torch.stack([torch.autograd.grad(qs[e].sum(), s["a"], retain_graph=True)[0] for e in range(len(members))])
    wrt = [v for v in actor_p.values() if v.requires_grad]
    grads = torch.autograd.grad(loss, wrt)
    stats = np.array([loss.item(), qs.detach().mean(dim=0).double().mean().item(), s["logp"].detach().double().mean().item(),
                      s["scale"].detach().double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, d_a=d_a.detach(), grads=list(grads), u=s["u"].detach(), a=s["a"].detach(),
                logp=s["logp"].detach(), q=qs.detach(), g_members=g_members.detach(), sample={k: v.detach() for k, v in s.items()})


def restate(case, n, dtype=torch.float64):
    """``loss_actor`` of one case on fresh leaves, with ``named`` = (state-dict name, gradient) in ``S.grad_names`` order."""
    a = S.leaf(actor_params(case), dtype)
    b = inputs(case, n)
    res = loss_actor(a, [member_params(case, e) for e in range(n_critics(case))], case, b["obs"], b["noise"], dtype=dtype)
    res["named"] = list(zip(S.grad_names(a), res["grads"]))
    return res


def restate_sequence(case=SEQ_CASE, n=SEQ_N):
    """One update in the reference agent's order (train_rlpd_agent.py:246-347) on ONE batch: ``SEQ_CRITIC_UPDATES`` times (the
    temperature's snapshot, critic loss, AdamW step, Polyak), then one actor loss with the last snapshot and its AdamW step, one
    temperature loss and its Adam step.  The critic loss's sample at next_obs and the pair are ``K.inputs``' and ``K.pair_of``'s in
    every repeat; the actor's draws are ``S.inputs``' ``noise``, the temperature's ``noise_t``.  Returns what
    make_golden_rlpd.update_sequence records."""
    E, b, sb = n_critics(case), K.inputs(case, n), S.inputs(sac_case(case), n)
    members = [K.leaf(K.member_params(case, e)) for e in range(E)]
    targets = [dict(K.member_params(case, e, K.TARGET_EPS)) for e in range(E)]
    a = S.leaf(actor_params(case))
    la = torch.tensor(SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_c = torch.optim.AdamW([t for p in members for t in p.values()], lr=SEQ_LR, weight_decay=SEQ_WEIGHT_DECAY)
    opt_a = torch.optim.AdamW([a[k] for k in S.grad_names(a)], lr=SEQ_ACTOR_LR, weight_decay=SEQ_WEIGHT_DECAY)
    opt_t = torch.optim.Adam([la], lr=SEQ_LR)
    out = dict(c_loss=[], gq=[])
    for _ in range(SEQ_CRITIC_UPDATES):
        alpha = float(la.detach().exp())
        rc = K.loss_critic(members, targets, case, b, K.pair_of(case, n), K.backup_entropy(case, n), alpha=alpha)
        for p, gs in zip(members, rc["grads"]):
            for t, g in zip(p.values(), gs):
                t.grad = g.clone()
        out["gq"].append([{k: t.grad.clone() for k, t in p.items()} for p in members])
        opt_c.step()
        for e in range(E):
            targets[e] = {k: targets[e][k] * (1.0 - SEQ_TAU) + members[e][k].detach() * SEQ_TAU for k in targets[e]}
        out["c_loss"].append(rc["loss"].item())
    stepped = [{k: t.detach() for k, t in p.items()} for p in members]
    ra = loss_actor(a, stepped, case, b["obs"], sb["noise"], alpha=alpha)
    for k, g in zip(S.grad_names(a), ra["grads"]):
        a[k].grad = g.clone()
    out["ga"] = {k: a[k].grad.clone() for k in S.grad_names(a)}
    opt_a.step()
    with torch.no_grad():
        logp = S.sample({k: v.detach() for k, v in a.items()}, sac_case(case), b["obs"], sb["noise_t"])["logp"]
    lt = -torch.mean(la.exp() * (logp + S.target_entropy(sac_case(case))))
    la.grad = torch.autograd.grad(lt, la)[0]
    opt_t.step()
    out.update(a_loss=ra["loss"].item(), t_loss=lt.item(), log_alpha=float(la.detach()), q=stepped, target=targets,
               actor={k: v.detach() for k, v in a.items()})
    return out
