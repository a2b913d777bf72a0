"""Case table and plain-torch restatement of Cal-QL's actor loss through the minimum of the LayerNorm twin (reference
model/rl/gaussian_calql.py:173-182), shared by make_golden_calql_actor.py (generator, needs the reference) and
tests/test_calql_actor.py (no reference needed).

Everything but two cases is borrowed from make_golden_calql_cases.py (``K``): the trunks, the actor, the observations and the
actor's draws (the ``pi`` segment of ``K.inputs(...)["noise"]``, so the sampled actions are ``K.samples(...)["pi_actions"]``).

K's twins are no test of a select: in float64 at those actions Q2 is the smaller on 1 % (tiny_77), 100 % (kitchen_256) and 21 %
(chunk_77) of the rows.  So a case here is (K's case, N, delta): ``delta``, a multiple of ``K.GRID``, is added to Q2's out-layer
bias, which moves q2 by exactly delta and nothing else.  The medians of q1 - q2 measured in float64 are -2.92 (tiny_77), -0.90
(chunk_77) and +2.16 (kitchen_256), the standard deviation 1.0 to 1.2; delta sits near the median (each trunk is selected on 40 to
60 % of the rows) but off it, so that no row sits on the boundary: the smallest float64 gap |q1 - q2| is at least 10 x FP32_Q_ERR,
the largest |q - q64| of the fp32 restatement on these rows (measure() prints both; tests/test_calql_actor.py asserts both
conditions).  ``tie``: both trunks carry Q1's weights, so q1 == q2 on every row and ``torch.min``'s backward halves.  ``wide``:
hidden 1024 (the top of LN_MAX_H) at N = 33 with a [64, 64] actor; no fixture holds it.

The restatement is written the way the reference writes it -- the sample, ``torch.min(q1, q2)``, ``(-min + alpha logp).mean()`` --
takes a dtype (float32 reproduces g30, float64 fed the same fp32 values is the yardstick of the GPU tests) and an optional ``sel``
handed in (0: Q1, 1: Q2, 2: both at one half), so that a second implementation is compared on ITS OWN decisions.  It works under
``K.relu_gates()`` and ``K.bf16_linears()``.

The recorded update sequence runs on K's own twin (delta = 0): ``K.returns_of`` is constructed with guard bands around K's Q
values, which a shifted Q2 would leave."""
import math

import numpy as np
import torch

from oracle import dppo_oracle as O
from tests.golden import make_golden_calql_cases as K

S = K.S
ALPHA, RANDN_CLIP = 0.7, S.RANDN_CLIP
# name -> (K's case, N, delta on Q2's out-layer bias; None: Q2 carries Q1's weights)
G = K.GRID
DELTA = {"tiny": -3072 * G, "chunk": -1024 * G, "kitchen": 2304 * G, "wide": -2304 * G}  # -3.0, -1.0, +2.25, -2.25
ACTOR_CASES = {
    "tiny_1_q1": ("tiny", 1, 0.0),      # q1 - q2 = -1.97: Q1
    "tiny_1_q2": ("tiny", 1, -4.0),     # Q2's bias lowered by 4: Q2
    "tiny_77": ("tiny", 77, DELTA["tiny"]),
    "chunk_77": ("chunk", 77, DELTA["chunk"]),   # Mish, Ta = 4
    "kitchen_256": ("kitchen", 256, DELTA["kitchen"]),
    "tie_77": ("tiny", 77, None),
}
WIDE = "wide_33"
WIDE_NET = (11, 1, 3, [1024, 1024], "ReLU")
WIDE_ACTOR_DIMS = [64, 64]
SEED_WIDE_Q, SEED_WIDE_ACTOR, SEED_WIDE_INPUTS = 3301, 3351, 3391
CASES = list(ACTOR_CASES)            # the fixture's
ALL_CASES = CASES + [WIDE]
BALANCED = ["tiny_77", "chunk_77", "kitchen_256"]  # conditions (a) and (b)
# the largest |q - q64| of the fp32 restatement over both trunks and the rows of BALANCED, measured on the CPU by measure():
# 1.79e-06 (chunk_77, rounded up); the smallest float64 gaps there: tiny_77 2.149e-02, chunk_77 9.119e-04, kitchen_256 3.033e-03; Q2 is selected
# on 52 %, 53 % and 46 % of the rows
FP32_Q_ERR = 1.79e-6
# the recorded update sequence (K's tiny, N = 77, delta = 0): one AdamW critic step with Polyak, one actor step, one temperature step
SEQ_CASE, SEQ_N = "tiny", 77
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU, SEQ_LOG_ALPHA, SEQ_WEIGHT_DECAY = 1e-3, 3e-4, 0.005, math.log(ALPHA), 0.0


def parts(case):
    """(K's case or "wide", N, delta)."""
    return ("wide", 33, DELTA["wide"]) if case == WIDE else ACTOR_CASES[case]


def net_of(case):
    """(obs_dim, Ta, Da, critic widths, activation)."""
    base = parts(case)[0]
    return WIDE_NET if base == "wide" else K.CALQL_NETS[base][:5]


def actor_dims(case):
    return list(WIDE_ACTOR_DIMS) if case == WIDE else list(net_of(case)[3])


def q_spec(case):
    od, ta, da, dims, act = net_of(case)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=list(dims), activation=act, residual=False, use_layernorm=True)


def out_bias_key(case, i=2):
    return f"Q{i}.moduleList.{len(net_of(case)[3])}.linear_1.bias"


def twin_params(case):
    """State dict of the case's CriticObsAct(use_layernorm=True, double_q=True): K's twin with delta on Q2's out-layer bias; ``tie``:
    Q2 := Q1; ``wide``: two seeded trunks of its own."""
    base, _, delta = parts(case)
    if base == "wide":
        q = {}
        for i in range(2):
            for k, v in O.init_params(q_spec(case), SEED_WIDE_Q + i, K.Q_SCALE).items():
                q[k.replace("Q1.", f"Q{i + 1}.")] = v
    else:
        q = dict(K.twin_params(base))
    if delta is None:
        return {k: (q[k.replace("Q2.", "Q1.")].clone() if k.startswith("Q2.") else v) for k, v in q.items()}
    key = out_bias_key(case)
    assert key in q and delta / K.GRID == round(delta / K.GRID)
    q[key] = q[key] + np.float32(delta)
    return q


def actor_params(case):
    """State dict of Gaussian_MLP(fixed_std=None, tanh_output=False): ``K.actor_params``; ``wide`` repeats its recipe on a [64, 64]
    base and a seed of its own."""
    base = parts(case)[0]
    if base != "wide":
        return K.actor_params(base)
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


def inputs(case):
    """dict(obs (n, 1, Do), noise (n, Ta, Da)): K's observations and the ``pi`` segment of its draws; ``wide`` draws its own."""
    base, n, _ = parts(case)
    if base != "wide":
        b, (_, Sn) = K.inputs(base, n), K.n_samples(base)
        return dict(obs=b["obs"], noise=b["noise"][n * Sn:n * Sn + n])
    od, ta, da = WIDE_NET[:3]
    rs = np.random.RandomState(SEED_WIDE_INPUTS)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(n, 1, od)).astype(np.float32))
    z = np.clip(rs.randn(n, ta, da), -S.NOISE_CAP, S.NOISE_CAP)
    return dict(obs=obs, noise=torch.from_numpy(z.astype(np.float32)))


def temperature_noise(case=SEQ_CASE, n=SEQ_N):
    """The temperature loss's draws in the sequence: the ``pi_next`` segment of K's."""
    _, Sn = K.n_samples(case)
    return K.inputs(case, n)["noise"][n * Sn + n:]


def sample(actor_p, case, obs, noise):
    """``S.sample`` on this case's actor: dict(a, u, logp, mean, raw, scale)."""
    base = parts(case)[0]
    if base == "wide":
        return S.sample(actor_p, "tiny", obs, noise)  # S's tiny IS a [64, 64] ReLU actor on 11 -> 3
    with K._lent(base) as key:
        return S.sample(actor_p, key, obs, noise)


def q_forward(p, case, obs, act):
    """One trunk's Q (n,) under the single critic's names."""
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    return O.critic_forward(p, q_spec(case), x).reshape(-1)


def select(q1, q2):
    """The kernel's rule as codes (n,) int64: 1 where q2 < q1, 2 where q1 == q2, 0 elsewhere."""
    one, two, zero = torch.ones_like(q1, dtype=torch.int64), torch.full_like(q1, 2, dtype=torch.int64), torch.zeros_like(q1, dtype=torch.int64)
    return torch.where(q2 < q1, one, torch.where(q1 == q2, two, zero))


def loss_actor(actor_p, q, case, obs, noise, alpha=ALPHA, dtype=torch.float32, sel=None):
    """gaussian_calql.py:173-182 with rsample's draw replaced by ``noise``.  ``actor_p``: leaf tensors of ``dtype``; ``q``: a plain
    twin dict.  ``sel`` (n,) codes given: row n takes q2 where 1, (q1 + q2) / 2 where 2, q1 where 0, instead of ``torch.min``.
    Returns dict(loss, stats {loss, mean q_sel, mean logp, mean sigma}, d_a = d mean(-q_sel) / d a, grads (one per entry of actor_p
    that takes a gradient, in its order), a, u, logp, q1, q2, sel (own codes), g = (dq1/da, dq2/da), sample)."""
    obs = obs.to(dtype)
    s = sample(actor_p, case, obs, noise)
    q = K.RL.cast(q, dtype)
    q1, q2 = (q_forward(K.trunk(q, i), case, obs, s["a"]) for i in (1, 2))
    own = select(q1.detach(), q2.detach())
    if sel is None:
        qs = torch.min(q1, q2)
    else:
        use = torch.as_tensor(np.asarray(sel)).reshape(-1).long()
        qs = torch.where(use == 1, q2, torch.where(use == 2, 0.5 * q1 + 0.5 * q2, q1))
    loss = (-qs + alpha * s["logp"]).mean()
    d_a = torch.autograd.grad((-qs).mean(), s["a"], retain_graph=True)[0]
    g = tuple(torch.autograd.grad(x.sum(), s["a"], retain_graph=True)[0].detach() for x in (q1, q2))
    wrt = [v for v in actor_p.values() if v.requires_grad]
    grads = torch.autograd.grad(loss, wrt)
    stats = np.array([loss.item(), qs.detach().double().mean().item(), s["logp"].detach().double().mean().item(),
                      s["scale"].detach().double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, d_a=d_a.detach(), grads=list(grads), a=s["a"].detach(), u=s["u"].detach(),
                logp=s["logp"].detach(), q1=q1.detach(), q2=q2.detach(), sel=own.numpy(), g=g,
                sample={k: v.detach() for k, v in s.items()})


def restate(case, dtype=torch.float64, sel=None):
    """``loss_actor`` of one case on fresh leaves, with ``named`` = (state-dict name, gradient) in ``S.grad_names`` order."""
    a, b = S.leaf(actor_params(case), dtype), inputs(case)
    res = loss_actor(a, twin_params(case), case, b["obs"], b["noise"], dtype=dtype, sel=sel)
    res["named"] = list(zip(S.grad_names(a), res["grads"]))
    return res


def restate_sequence(case=SEQ_CASE, n=SEQ_N):
    """One update in the agent's order (reference train_calql_agent.py:408-445) on ONE batch of K's ``case``: the temperature's
    snapshot, the critic loss (K.loss_critic on K's samples and constructed returns), its AdamW step, Polyak, the actor loss with the
    snapshot and the STEPPED critic, its AdamW step, the temperature loss and its Adam step.  Returns what
    make_golden_calql_actor.update_sequence records."""
    b, sm = K.inputs(case, n), K.samples(case, n)
    _, Sn = K.n_samples(case)
    q, tq, a = K.RL.leaf(K.twin_params(case)), dict(K.twin_params(case, K.TARGET_EPS)), S.leaf(K.actor_params(case))
    la = torch.tensor(SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_c = torch.optim.AdamW(list(q.values()), lr=SEQ_LR, weight_decay=SEQ_WEIGHT_DECAY)
    opt_a = torch.optim.AdamW([a[k] for k in S.grad_names(a)], lr=SEQ_ACTOR_LR, weight_decay=SEQ_WEIGHT_DECAY)
    opt_t = torch.optim.Adam([la], lr=SEQ_LR)
    alpha = float(la.detach().exp())
    rc = K.loss_critic(q, tq, case, b, sm, K.returns_of(case, n), clips=K.clips_of(case, n))
    for t, g in zip(q.values(), rc["grads"]):
        t.grad = g.clone()
    gq = {k: t.grad.clone() for k, t in q.items()}
    opt_c.step()
    stepped = {k: t.detach() for k, t in q.items()}
    target = {k: tq[k] * (1.0 - SEQ_TAU) + stepped[k] * SEQ_TAU for k in tq}
    noise = b["noise"][n * Sn:n * Sn + n]
    # (the case name serves loss_actor only for the shapes: tiny_77 is K's tiny at N = 77)
    ra = loss_actor(a, stepped, f"{case}_{n}", b["obs"], noise, alpha=alpha)
    for k, g in zip(S.grad_names(a), ra["grads"]):
        a[k].grad = g.clone()
    ga = {k: a[k].grad.clone() for k in S.grad_names(a)}
    opt_a.step()
    with torch.no_grad():
        logp = sample({k: v.detach() for k, v in a.items()}, f"{case}_{n}", b["obs"], temperature_noise(case, n))["logp"]
    _, ta, da = K.shapes(case)
    lt = -torch.mean(la.exp() * (logp + (-float(ta * da))))
    la.grad = torch.autograd.grad(lt, la)[0]
    opt_t.step()
    return dict(c_loss=rc["loss"].item(), gq=gq, q=stepped, target=target, a_loss=ra["loss"].item(), ga=ga, t_loss=lt.item(),
                log_alpha=float(la.detach()), actor={k: v.detach() for k, v in a.items()})


def balance(case):
    """(share of rows that select Q2, smallest |q1 - q2|, largest fp32 |q - q64| over both trunks) of a case, in float64."""
    r64, r32 = restate(case, torch.float64), restate(case, torch.float32)
    gap = (r64["q1"] - r64["q2"]).abs().min().item()
    err = max((r32[k].double() - r64[k]).abs().max().item() for k in ("q1", "q2"))
    return float((r64["sel"] == 1).mean()), gap, err


def measure():
    worst = 0.0
    for case in ALL_CASES:
        share, gap, err = balance(case)
        r = restate(case)
        print(f"{case}: Q2 on {100 * share:.0f} %, median q1 - q2 {(r['q1'] - r['q2']).median().item():+.3f}, smallest gap {gap:.3e}, "
              f"largest fp32 |q - q64| {err:.3e}")
        if case in BALANCED:
            worst = max(worst, err)
    print(f"FP32_Q_ERR = {worst:.3e}")


if __name__ == "__main__":
    measure()
