"""Case table, seeded recipes and a plain-torch restatement shared by make_golden_sac.py (generator, needs the reference) and
tests/test_sac.py (no reference needed): SAC's tanh-Gaussian sample with its log-probability, the entropy-regularised TD loss, the
reparameterised actor loss, the temperature loss and one update sequence.

Nothing large is stored in g27_sac.npz: weights and inputs come from the seeded numpy recipes below; the fixture holds what only
the reference can say.  The restatement is written the way the reference writes it (``Normal.log_prob`` of the clamped draw,
``log(1 - a^2 + 1e-6)``), takes a dtype -- float32 reproduces the fixture, float64 fed the same fp32 values is the yardstick of the
GPU tests -- and an optional forced ``sel`` (which trunk is the smaller, per row), so that a second implementation is compared on
ITS OWN decisions.  ``bf16_linears`` / ``relu_gates`` are make_golden_dql_cases.py's contexts."""
import math

import numpy as np
import torch

from oracle import dppo_oracle as O
from tests.golden.make_golden_dql_cases import RELU_TIE, bf16_linears, relu_gates  # noqa: F401  (re-exported)

# case -> (obs_dim, Ta, Da, hidden widths of the actor's base AND of the critics, activation, noise scale, logvar head's weight scale)
SAC_NETS = {
    "cheetah": (17, 1, 6, [256, 256], "ReLU", 1.0, 1.0),   # gym/scratch/halfcheetah-v2/sac_mlp.yaml
    "tiny": (11, 1, 3, [64, 64], "ReLU", 1.0, 1.0),        # AF = 3: below one 16-byte store; 2 AF = 6
    "chunk": (22, 4, 7, [128, 128], "Mish", 1.0, 1.0),     # AF = 28, 2 AF = 56: not a multiple of 16 or 64
    # tiny with the draws scaled by 2.5 (|z| on both sides of the clip) and, since sigma z stays below 3 sigma, the logvar head's
    # weights scaled too: sigma from std_min-ish to about 5, |u| from 0 to about 12
    "tiny_sat": (11, 1, 3, [64, 64], "ReLU", 2.5, 4.0),
}
SIZES = (1, 77, 256)
CASES = [(c, n) for c in ("cheetah", "tiny", "chunk") for n in SIZES] + [("tiny_sat", 77)]
SAT_CASES = [("tiny_sat", 77)]
STD_MIN, STD_MAX = 0.0067, 7.3891   # the shipped cfg's
RANDN_CLIP = 3.0
NOISE_CAP = 2.5                     # non-sat draws are kept this far inside the clip
ALPHA, GAMMA = 0.7, 0.99
SEED_ACTOR, SEED_Q1, SEED_Q2, SEED_TARGET = 271, 272, 273, 274
Q_SCALE, TARGET_EPS = 3.0, 0.05     # as make_golden_qsm_cases.py: outputs and action gradients of O(1)
# guard bands (tests/test_sac.py asserts them on the float64 restatement): ten times the fp32 ceiling of the quantity
Q_CEIL, Z_CEIL = 1e-5, 1e-6          # |q| is O(1): 1e-5 is the statistics' tolerance class; z is an input, exact up to its own ulp
U_MAX = 2.0
# the recorded update sequence (cheetah, N = 77): Adam(lr, betas (0.9, 0.999), eps 1e-8) steps
SEQ_LR, SEQ_ACTOR_LR, SEQ_TAU, SEQ_LOG_ALPHA = 1e-3, 3e-4, 0.005, math.log(ALPHA)


def shapes(case):
    """(obs_dim, Ta, Da) of a case."""
    return SAC_NETS[case][:3]


def dims(case):
    return list(SAC_NETS[case][3])


def activation(case):
    return SAC_NETS[case][4]


def target_entropy(case):
    _, ta, da = shapes(case)
    return -float(ta * da)


def logvar_bounds():
    """log std_min^2, log std_max^2 as the reference's fp32 parameters hold them."""
    return (torch.log(torch.tensor(STD_MIN ** 2)), torch.log(torch.tensor(STD_MAX ** 2)))


def q_spec(case):
    od, ta, da = shapes(case)
    return O.NetSpec("critic", cond_dim=od + ta * da, mlp_dims=dims(case), activation=activation(case), residual=False)


def actor_params(case):
    """State dict of Gaussian_MLP(fixed_std=None, tanh_output=False), in the reference's order."""
    od, ta, da = shapes(case)
    base = case.split("_")[0]  # tiny_sat shares tiny's weights
    d, rs = dims(case), np.random.RandomState(SEED_ACTOR + 10 * list(SAC_NETS).index(base))
    lmin, lmax = logvar_bounds()
    p = {"logvar_min": lmin, "logvar_max": lmax}

    def lin(name, i, o, scale=1.0):
        b = scale / math.sqrt(i)
        p[f"{name}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(o, i)).astype(np.float32))
        p[f"{name}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(o,)).astype(np.float32))
    widths = [od] + d
    for i in range(len(widths) - 1):
        lin(f"mlp_base.moduleList.{i}.linear_1", widths[i], widths[i + 1])
    lin("mlp_mean.moduleList.0.linear_1", d[-1], ta * da)
    lin("mlp_logvar.moduleList.0.linear_1", d[-1], ta * da, SAC_NETS[case][6])
    return p


def twin_params(case, eps=0.0):
    """State dict of CriticObsAct (plain trunks): Q1 and Q2 from distinct seeds; eps != 0 adds the target's perturbation."""
    base = case.split("_")[0]
    spec, out, k = q_spec(case), {}, 10 * list(SAC_NETS).index(base)
    for i, seed in enumerate((SEED_Q1, SEED_Q2)):
        p, d = O.init_params(spec, seed + k, Q_SCALE), O.init_params(spec, SEED_TARGET + k + 100 * i, Q_SCALE)
        for key in p:
            out[key.replace("Q1.", f"Q{i + 1}.")] = p[key] + np.float32(eps) * d[key] if eps else p[key]
    return out


def inputs(case, n):
    """The n seeded transitions of a case and every draw the losses take from outside.  noise: the actor loss's; noise_next: the
    critic loss's sample at next_obs; noise_t: the temperature loss's; noise2 / noise_t2: the sequence's second actor / temperature
    update.  Draws are N(0, 1) times the case's noise scale; outside the ``sat`` case they are clamped to +-NOISE_CAP."""
    od, ta, da = shapes(case)
    scale = SAC_NETS[case][5]
    rs = np.random.RandomState(2700 + 13 * list(SAC_NETS).index(case) + n)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, nxt, act = f(n, 1, od), f(n, 1, od), f(n, ta, da)
    reward = torch.from_numpy(rs.uniform(0, 4, size=n).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=n) < 0.3).astype(np.float32))

    def z():
        x = scale * rs.randn(n, ta, da)
        if case not in dict(SAT_CASES):
            x = np.clip(x, -NOISE_CAP, NOISE_CAP)
        return torch.from_numpy(x.astype(np.float32))
    return dict(obs=obs, next_obs=nxt, actions=act, reward=reward, terminated=terminated, noise=z(), noise_next=z(), noise_t=z(),
                noise2=z(), noise_t2=z())


def leaf(params, dtype=torch.float32):
    return {k: v.to(dtype).clone().requires_grad_(not k.startswith("logvar_m")) for k, v in params.items()}


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def heads(p, case, obs):
    """(mean, raw logvar, scale), each (n, AF): mlp_gaussian.py:348-379 with tanh_output=False."""
    act = lambda x: O._ACT[activation(case)](x)  # (looked up per call: relu_gates swaps the entry)
    x = obs.reshape(len(obs), -1)
    h = act(O._plain_mlp(p, "mlp_base", x, len(dims(case)), act, False))
    lin = lambda name: torch.nn.functional.linear(h, p[f"{name}.moduleList.0.linear_1.weight"], p[f"{name}.moduleList.0.linear_1.bias"])
    mean, raw = lin("mlp_mean"), lin("mlp_logvar")
    lv = torch.tanh(raw)
    lv = p["logvar_min"] + 0.5 * (p["logvar_max"] - p["logvar_min"]) * (lv + 1)
    return mean, raw, torch.exp(0.5 * lv)


def sample(p, case, obs, noise, deterministic=False, squash=True):
    """gaussian.py:85-120 with rsample's draw replaced by ``noise``: dict(a, u, logp, mean, raw, scale), a and u (n, AF)."""
    mean, raw, scale = heads(p, case, obs)
    if deterministic:
        scale = torch.ones_like(mean) * 1e-4
    x = mean + noise.reshape(mean.shape).to(mean.dtype) * scale
    x = torch.max(torch.min(x, mean + RANDN_CLIP * scale), mean - RANDN_CLIP * scale)
    var = scale ** 2
    logp = -((x - mean) ** 2) / (2 * var) - scale.log() - math.log(math.sqrt(2 * math.pi))
    a = x
    if squash:
        a = torch.tanh(x)
        logp = logp - torch.log(1 - a.pow(2) + 1e-6)
    return dict(a=a, u=x, logp=logp.sum(1), mean=mean, raw=raw, scale=scale)


def twin_forward(q, case, obs, act):
    spec = q_spec(case)
    x = torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)
    trunk = lambda i: {k.replace(f"Q{i}.", "Q1."): v for k, v in q.items() if k.startswith(f"Q{i}.")}
    return tuple(O.critic_forward(trunk(i), spec, x).reshape(-1) for i in (1, 2))


def _to(b, dtype):
    return {k: v.to(dtype) for k, v in b.items()}


def loss_critic(q, tq, actor_p, case, b, alpha=ALPHA, dtype=torch.float32, noise_key="noise_next"):
    """gaussian_sac.py:31-59.  q: leaf tensors of ``dtype``.  Returns dict(loss, stats {loss, mean q1, mean y}, next_a, next_logp, grads)."""
    b, tq, actor_p = _to(b, dtype), cast(tq, dtype), cast(actor_p, dtype)
    with torch.no_grad():
        s = sample(actor_p, case, b["next_obs"], b[noise_key])
        nq = torch.min(*twin_forward(tq, case, b["next_obs"], s["a"])) - alpha * s["logp"]
        y = b["reward"] + GAMMA * nq * (1 - b["terminated"])
    q1, q2 = twin_forward(q, case, b["obs"], b["actions"])
    loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
    grads = torch.autograd.grad(loss, list(q.values()))
    stats = np.array([loss.item(), q1.detach().double().mean().item(), y.double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, next_a=s["a"], next_logp=s["logp"], grads=list(grads))


def loss_actor(actor_p, q, case, b, alpha=ALPHA, dtype=torch.float32, sel=None, noise_key="noise", squash=True):
    """gaussian_sac.py:61-70.  actor_p: leaf tensors of ``dtype``.  sel (n,) bool given: row n takes q2 where sel, q1 elsewhere,
    instead of torch.min.  squash=False: ``GaussianModel.tanh_output=False`` (a = u, no log-det term).  Returns dict(loss, stats {loss, mean q_sel, mean logp, mean sigma}, a, u, logp, q1, q2, sel, d_a =
    d mean(-q_sel) / d a, grads (one per entry of actor_p that takes a gradient, in its order), sample)."""
    b, q = _to(b, dtype), cast(q, dtype)
    s = sample(actor_p, case, b["obs"], b[noise_key], squash=squash)
    q1, q2 = twin_forward(q, case, b["obs"], s["a"])
    own = (q2 < q1).detach()
    use = own if sel is None else torch.as_tensor(sel).reshape(-1).bool()
    qs = torch.where(use, q2, q1)
    loss = (-qs + alpha * s["logp"]).mean()
    d_a = torch.autograd.grad((-qs).mean(), s["a"], retain_graph=True)[0]
    wrt = [v for v in actor_p.values() if v.requires_grad]
    grads = torch.autograd.grad(loss, wrt)
    stats = np.array([loss.item(), qs.detach().double().mean().item(), s["logp"].detach().double().mean().item(),
                      s["scale"].detach().double().mean().item()])
    return dict(loss=loss.detach(), stats=stats, a=s["a"].detach(), u=s["u"].detach(), logp=s["logp"].detach(), q1=q1.detach(),
                q2=q2.detach(), sel=own.numpy(), d_a=d_a.detach(), grads=list(grads), sample={k: v.detach() for k, v in s.items()})


def grad_names(actor_p):
    return [k for k, v in actor_p.items() if not k.startswith("logvar_m")]


def loss_temperature(actor_p, case, b, log_alpha, dtype=torch.float32, noise_key="noise_t"):
    """gaussian_sac.py:72-80 with alpha = exp(log_alpha) -> (loss, d loss / d log_alpha, logp)."""
    b, actor_p = _to(b, dtype), cast(actor_p, dtype)
    la = torch.tensor(float(log_alpha), dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        logp = sample(actor_p, case, b["obs"], b[noise_key])["logp"]
    loss = -torch.mean(la.exp() * (logp + target_entropy(case)))
    g = torch.autograd.grad(loss, la)[0]
    return loss.detach(), g, logp


def head_backward(s, g, zc, alpha, n, lmin, lmax):
    """The analytic head gradient the kernels implement: (d loss / d mean, d loss / d raw) from g = dQ_sel/da."""
    a, sigma, raw = s["a"], s["scale"], s["raw"]
    sq = 1 - a ** 2
    du = (-g * sq + alpha * 2 * a * sq / (sq + 1e-6)) / n
    dsig = du * zc - alpha / (n * sigma)
    draw = dsig * 0.5 * sigma * 0.5 * (lmax - lmin) * (1 - torch.tanh(raw) ** 2)
    return du, draw


def restate_sequence(case="cheetah", n=77):
    """One update in the reference agent's order (:242-280): alpha's snapshot, critic loss and Adam step, Polyak, then twice: actor
    loss with the snapshot and the UPDATED critic, Adam step, temperature loss and Adam step.  Returns what
    make_golden_sac.update_sequence records."""
    b = inputs(case, n)
    q, tq, a = leaf(twin_params(case)), twin_params(case, TARGET_EPS), leaf(actor_params(case))
    la = torch.tensor(SEQ_LOG_ALPHA, dtype=torch.float64, requires_grad=True)
    opt_c = torch.optim.Adam(list(q.values()), lr=SEQ_LR)
    opt_a = torch.optim.Adam([a[k] for k in grad_names(a)], lr=SEQ_ACTOR_LR)
    opt_t = torch.optim.Adam([la], lr=SEQ_LR)
    alpha = float(la.detach().exp())
    rc = loss_critic(q, tq, {k: v.detach() for k, v in a.items()}, case, b, alpha)
    for v, g in zip(q.values(), rc["grads"]):
        v.grad = g.clone()
    gq = {k: v.grad.clone() for k, v in q.items()}
    opt_c.step()
    q2 = {k: v.detach() for k, v in q.items()}
    t2 = {k: tq[k] * (1.0 - SEQ_TAU) + q2[k] * SEQ_TAU for k in tq}
    out = dict(c_loss=rc["loss"].item(), gq=gq, q=q2, target=t2, a_loss=[], t_loss=[], ga=[], log_alpha=[])
    for nk, tk in (("noise", "noise_t"), ("noise2", "noise_t2")):
        ra = loss_actor(a, q2, case, b, alpha, noise_key=nk)
        for k, g in zip(grad_names(a), ra["grads"]):
            a[k].grad = g.clone()
        out["ga"].append({k: a[k].grad.clone() for k in grad_names(a)})
        opt_a.step()
        lt, g, _ = loss_temperature({k: v.detach() for k, v in a.items()}, case, b, la.detach(), noise_key=tk)
        la.grad = g.clone().reshape(la.shape)
        opt_t.step()
        out["a_loss"].append(ra["loss"].item())
        out["t_loss"].append(lt.item())
        out["log_alpha"].append(float(la.detach()))
    out["actor"] = {k: v.detach() for k, v in a.items()}
    return out
