"""Time RLPD's updates (batch 256) at the shipped halfcheetah shape (E = 10, hidden [256, 256], Ta*Da = 6, 20 critic updates per
iteration) and at the can shape (E = 5, hidden [256, 256, 256], actor [512, 512, 512], Ta*Da = 7, 3 critic updates per iteration), bf16
and fp32.  Arms are named on the command line (none: ``update``):

    python3 tools/rlpd_bench.py profiles/rlpd_update.json
    python3 tools/rlpd_bench.py profiles/rlpd_iteration.json actor iteration

The ``update`` arm:
  critic  one critic update of RLPD_Gaussian out of plain tensors with the policy's sample at the next observations given:
          loss_critic (dppo_rlpd_q_loss_fwd_bwd: two target members, all E members forward and backward), one FlatAdamW step over the
          [E][P] image, one Polyak call;
  eager   the same update as plain torch on the same GPU: the reference's arithmetic with torch.func.stack_module_state /
          functional_call / vmap over the members, torch.optim.Adam over the stacked parameters, Polyak per parameter, fp32, and one
          ``.item()`` per update as the reference agent takes;
  E = 2   the critic arm again with two members, the fewest the call takes: how one update's time divides between the per-call part
          and the per-member part, the evidence for or against a member-batched GEMM.
The ``actor`` arm: one actor update (loss_actor = dppo_rlpd_actor_fwd_bwd: the actor's forward, E member forwards and action-gradient
chains, the tail, the actor's backward; one FlatAdamW step) against the same in plain torch (rsample, vmap over the members, mean,
backward, Adam).  The ``iteration`` arm: what one training iteration of the agent queues behind its rollout, ``critic_num_update``
critic updates as above with the temperature's device snapshot, then one actor update and one temperature update (a fresh sample,
dppo_sac_alpha_loss, torch.optim.Adam on the device scalar), against the same iteration in plain torch with one ``.item()`` per
critic update.  Batches are given (the two index draws and gathers of the agent are not timed on either side).
Every arm is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported
(tools/idql_bench.timed).  First measurements of a new path: no threshold is set."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

from tools.idql_bench import measured_on, timed  # noqa: E402

DEV, N, GAMMA, ALPHA, TAU, LR = "cuda:0", 256, 0.99, 0.7, 0.005, 3e-4
SHAPES = {"cheetah": dict(od=17, ta=1, da=6, dims=[256, 256], actor=[256, 256], act="ReLU", E=10, updates=20),
          "can": dict(od=23, ta=1, da=7, dims=[256, 256, 256], actor=[512, 512, 512], act="ReLU", E=5, updates=3)}
STD_MIN, STD_MAX, CLIP = 0.0067, 7.3891, 3.0


def make_model(shape, prec, E):
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_rlpd import RLPD_Gaussian
    s = SHAPES[shape]
    actor = Gaussian_MLP(s["da"], s["ta"], s["od"], mlp_dims=s["actor"], activation_type=s["act"], tanh_output=False, fixed_std=None,
                         std_min=STD_MIN, std_max=STD_MAX, precision=prec)
    critic = CriticObsAct(cond_dim=s["od"], mlp_dims=s["dims"], action_dim=s["da"], action_steps=s["ta"], activation_type=s["act"],
                          use_layernorm=True, double_q=False, precision=prec)
    return RLPD_Gaussian(actor=actor, critic=critic, n_critics=E, backup_entropy=True, horizon_steps=s["ta"], device=DEV,
                         randn_clip_value=3.0, tanh_output=True)


def batches(shape, count=16):
    s = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(0)
    u = lambda *sz: torch.rand(*sz, device=DEV, generator=g) * 2 - 1
    return [dict(obs=u(N, 1, s["od"]), next_obs=u(N, 1, s["od"]), actions=u(N, s["ta"], s["da"]), reward=u(N) + 1,
                 terminated=(u(N) > 0.9).float(), next_actions=u(N, s["ta"], s["da"]), next_logp=u(N) - 1) for _ in range(count)]


def hip_update(model, data, alpha_of=None):
    from dppo_amd.util.optim import FlatAdamW
    opt = FlatAdamW(model.critic_flat_params(), lr=LR, weight_decay=0.0)
    fixed = torch.full((1,), ALPHA, dtype=torch.float64, device=DEV)
    it = iter(range(10 ** 9))

    def step():
        b = data[next(it) % len(data)]
        alpha = fixed if alpha_of is None else alpha_of()
        model.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], GAMMA, alpha,
                          next_actions=b["next_actions"], next_logp=b["next_logp"])
        opt.step(model.critic_flat_grads())
        model.critics_updated()
        model.update_target_critic(TAU)
    return step


def hip_actor(model, data, alpha_of=None):
    from dppo_amd.util.optim import FlatAdamW
    opt = FlatAdamW(model.network.flat_params(), lr=LR, weight_decay=0.0)
    fixed = torch.full((1,), ALPHA, dtype=torch.float64, device=DEV)
    it = iter(range(10 ** 9))

    def step():
        b = data[next(it) % len(data)]
        model.loss_actor({"state": b["obs"]}, fixed if alpha_of is None else alpha_of())
        opt.step(model.last_loss_grad)
        model.network.mark_updated()
    return step


def hip_iteration(model, data, shape):
    """The agent's update_iteration on given batches: critic updates with the snapshot, one actor update, one temperature update."""
    s = SHAPES[shape]
    log_alpha = torch.tensor(0.0, dtype=torch.float64, device=DEV, requires_grad=True)
    opt_t = torch.optim.Adam([log_alpha], lr=LR)
    snap = [None]
    critic, actor = hip_update(model, data, lambda: snap[0]), hip_actor(model, data, lambda: snap[0])

    def step():
        for _ in range(s["updates"]):
            snap[0] = log_alpha.detach().exp()
            critic()
        actor()
        opt_t.zero_grad()
        model.loss_temperature({"state": data[0]["obs"]}, log_alpha, -float(s["ta"] * s["da"])).backward()
        opt_t.step()
    return step


class _Actor(nn.Module):
    """Gaussian_MLP(fixed_std=None, tanh_output=False) as plain torch, and GaussianModel.forward's squashed sample."""

    def __init__(self, s):
        super().__init__()
        dims, layers = [s["od"]] + s["actor"], []
        for i in range(len(dims) - 1):
            layers += [nn.Linear(dims[i], dims[i + 1]), getattr(nn, s["act"])()]
        self.base = nn.Sequential(*layers)
        self.mean, self.logvar = nn.Linear(dims[-1], s["ta"] * s["da"]), nn.Linear(dims[-1], s["ta"] * s["da"])
        self.lmin, self.lmax = 2 * torch.log(torch.tensor(STD_MIN)).item(), 2 * torch.log(torch.tensor(STD_MAX)).item()

    def forward(self, obs):
        h = self.base(obs.reshape(len(obs), -1))
        mean, lv = self.mean(h), torch.tanh(self.logvar(h))
        scale = torch.exp(0.5 * (self.lmin + 0.5 * (self.lmax - self.lmin) * (lv + 1)))
        dist = torch.distributions.Normal(mean, scale)
        x = dist.rsample()
        x = torch.max(torch.min(x, mean + CLIP * scale), mean - CLIP * scale)
        a = torch.tanh(x)
        return a, (dist.log_prob(x) - torch.log(1 - a.pow(2) + 1e-6)).sum(1)


class _Member(nn.Module):
    def __init__(self, dims, act):
        super().__init__()
        layers = []
        for i in range(len(dims) - 2):
            layers += [nn.Linear(dims[i], dims[i + 1]), nn.LayerNorm(dims[i + 1]), getattr(nn, act)()]
        self.net = nn.Sequential(*layers, nn.Linear(dims[-2], dims[-1]))

    def forward(self, obs, act):
        return self.net(torch.cat([obs.reshape(len(obs), -1), act.reshape(len(act), -1)], dim=-1)).squeeze(-1)


def eager_update(shape, data):
    return eager_parts(shape, data)["critic"]


def eager_parts(shape, data):
    """The reference's three updates as plain torch on one set of networks: dict(critic, actor, temperature, iteration)."""
    s = SHAPES[shape]
    dims = [s["od"] + s["ta"] * s["da"]] + s["dims"] + [1]
    members = [_Member(dims, s["act"]).to(DEV) for _ in range(s["E"])]
    targets = [copy.deepcopy(m) for m in members]
    base = copy.deepcopy(members[0]).to("meta")
    params, buffers = torch.func.stack_module_state(members)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(params.values()), lr=LR)
    log_alpha = torch.tensor(0.0, device=DEV)
    call = lambda p, bf, x: torch.func.functional_call(base, (p, bf), x)
    it = iter(range(10 ** 9))

    def step():
        b = data[next(it) % len(data)]
        alpha = log_alpha.exp().item()
        i, j = torch.randperm(s["E"])[:2].tolist()
        with torch.no_grad():
            nq = torch.min(targets[i](b["next_obs"], b["next_actions"]), targets[j](b["next_obs"], b["next_actions"]))
            y = b["reward"] + GAMMA * (1 - b["terminated"]) * nq
            y = y + GAMMA * (1 - b["terminated"]) * alpha * (-b["next_logp"])
        q = torch.vmap(call, in_dims=(0, 0, None))(params, buffers, (b["obs"], b["actions"]))
        loss = torch.mean((q - y[None]) ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            for e, t in enumerate(targets):
                for k, p in t.named_parameters():
                    p.copy_(p * (1.0 - TAU) + params[k][e] * TAU)
    policy = _Actor(s).to(DEV)
    opt_a = torch.optim.Adam(policy.parameters(), lr=LR)
    log_alpha.requires_grad_(True)
    opt_t = torch.optim.Adam([log_alpha], lr=LR)
    te = -float(s["ta"] * s["da"])

    def actor_step():
        b = data[next(it) % len(data)]
        alpha = log_alpha.detach().exp()
        a, logp = policy(b["obs"])
        q = torch.vmap(call, in_dims=(0, 0, None))(params, buffers, (b["obs"], a.reshape(len(a), s["ta"], s["da"])))
        loss = -torch.mean(q.mean(dim=0) + alpha * (-logp))
        opt_a.zero_grad()
        loss.backward()
        opt_a.step()

    def temperature_step():
        with torch.no_grad():
            _, logp = policy(data[0]["obs"])
        loss = -torch.mean(log_alpha.exp() * (logp + te))
        opt_t.zero_grad()
        loss.backward()
        opt_t.step()

    def iteration():
        for _ in range(s["updates"]):
            step()
        actor_step()
        temperature_step()
    return dict(critic=step, actor=actor_step, temperature=temperature_step, iteration=iteration)


def arm(out, shape, what, unit):
    """One of the new arms at the shape's own E: hip in both precisions, eager, and the ratio."""
    s, data = SHAPES[shape], batches(shape)
    make = dict(actor=hip_actor, iteration=lambda m, d: hip_iteration(m, d, shape))[what]
    eag, reps = timed(eager_parts(shape, data)[what])
    out[f"{shape}/{what}/eager_torch_fp32"] = {unit: eag, "per_pass": reps}
    print(shape, what, "eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        ms, reps = timed(make(make_model(shape, prec, s["E"]), data))
        out[f"{shape}/{what}/{prec}"] = {unit: ms, "per_pass": reps, "eager_over_hip": eag / ms}
        print(shape, what, prec, ms, flush=True)


def main(path, arms):
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(), batch=N,
               method="median of 10 passes of >= 0.5 s between device events, every arm warmed")
    for shape, s in SHAPES.items():
        if "actor" in arms:
            arm(out, shape, "actor", "ms_per_actor_update")
        if "iteration" in arms:
            out[f"{shape}/iteration/critic_updates"] = s["updates"]
            arm(out, shape, "iteration", "ms_per_iteration")
        if "update" not in arms:
            continue
        data = batches(shape)
        for prec in ("bf16", "fp32"):
            for E in (s["E"], 2):
                ms, reps = timed(hip_update(make_model(shape, prec, E), data))
                out[f"{shape}/{prec}/E={E}"] = dict(ms_per_critic_update=ms, updates_per_pass=reps)
                print(shape, prec, E, ms, flush=True)
        eag, reps = timed(eager_update(shape, data))
        out[f"{shape}/eager_torch_fp32/E={s['E']}"] = dict(ms_per_critic_update=eag, updates_per_pass=reps)
        for prec in ("bf16", "fp32"):
            out[f"{shape}/{prec}/E={s['E']}"]["eager_over_hip"] = eag / out[f"{shape}/{prec}/E={s['E']}"]["ms_per_critic_update"]
        print(shape, "eager", eag, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], set(sys.argv[2:]) or {"update"})
