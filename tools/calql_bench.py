"""Time Cal-QL at the shipped kitchen shape (batch 256, obs 60, Ta*Da = 9, twin of [256, 256, 256] ReLU LayerNorm trunks, 10 random
actions and 10 policy samples per row), bf16 and fp32:

    python3 tools/calql_bench.py profiles/calql_loss_critic.json            (the critic arm)
    python3 tools/calql_bench.py actor profiles/calql_actor.json
    python3 tools/calql_bench.py iteration profiles/calql_iteration.json

The critic arm:

  hip     CalQL_Gaussian.loss_critic out of plain tensors with the policy's three samples given (dppo_calql_q_loss_fwd_bwd: the row
          builder, the two target trunks on N S rows, both trunks forward and backward ONCE on N (R + 3) rows, the target, loss and
          statistics kernels) -- the gradient is left in critic.flat_grads(); no optimiser step on either side;
  draws   the same with random_actions=None: the kernel draws them (one CPU-generator seed per call);
  eager   the restatement of tests/golden/make_golden_calql_cases.py (loss_critic, fp32) as plain torch on the same GPU with the
          same samples given, and torch.autograd.grad over both trunks' parameters.
The ``actor`` arm: CalQL_Gaussian.loss_actor (dppo_calql_actor_fwd_bwd; make_golden_calql_actor_cases.py's kitchen_256 twin, which
selects each trunk on about half of the rows) with the draws given, against the eager restatement (the sample, both trunks, torch.min,
the loss) with torch.autograd.grad over the actor's parameters; no optimiser step on either side.
The ``iteration`` arm: one full update as the agent runs it -- TrainCalQLAgent.update_iteration on a given batch: the policy's
samples and the random actions drawn, critic loss, FlatAdamW step, Polyak, actor loss, FlatAdamW step, temperature loss and Adam step
-- against the same steps in eager torch (torch.optim.AdamW on the parameter tensors, lerp_ for Polyak).
Every arm is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported
(tools/idql_bench.timed).  The launch counts are csrc/calql.h's (read off the code).  First measurements of a new path: no
threshold is set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.golden import make_golden_calql_actor_cases as A  # noqa: E402
from tests.golden import make_golden_calql_cases as K  # noqa: E402
from tools.idql_bench import measured_on, timed  # noqa: E402

DEV, CASE, N = "cuda:0", "kitchen", 256


def make_model(prec):
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_calql import CalQL_Gaussian
    od, ta, da, dims, act, R, S = K.CALQL_NETS[CASE]
    actor = Gaussian_MLP(da, ta, od, mlp_dims=dims, activation_type=act, tanh_output=False, fixed_std=None, std_min=K.S.STD_MIN,
                         std_max=K.S.STD_MAX, precision=prec)
    critic = CriticObsAct(cond_dim=od, mlp_dims=dims, action_dim=da, action_steps=ta, activation_type=act, use_layernorm=True,
                          double_q=True, twin_layernorm=True, precision=prec)
    m = CalQL_Gaussian(actor=actor, critic=critic, cql_min_q_weight=K.MIN_Q_WEIGHT, cql_n_actions=S, horizon_steps=ta, device=DEV,
                       randn_clip_value=K.S.RANDN_CLIP, tanh_output=True)
    m.critic.load_state_dict(K.twin_params(CASE), strict=True)
    m.target_critic.load_state_dict(K.twin_params(CASE, K.TARGET_EPS), strict=True)
    m.n_random_actions = R
    return m


def hip_step(model, b, sm, ret, draws=False):
    def step():
        model.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], None if draws else b["random_actions"], b["reward"],
                          ret, b["terminated"], K.GAMMA, samples=sm)
    return step


def eager_step(b, sm, ret):
    q = {k: v.to(DEV).clone().requires_grad_(True) for k, v in K.twin_params(CASE).items()}
    tq = {k: v.to(DEV) for k, v in K.twin_params(CASE, K.TARGET_EPS).items()}

    def step():
        K.loss_critic(q, tq, CASE, b, sm, ret, host_stats=False)
    return step


METHOD = "median of 10 passes of >= 0.5 s between device events, every arm warmed"


def header(**kw):
    return dict(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(), batch=N, method=METHOD), **kw)


def write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main(path):
    b = {k: v.to(DEV) for k, v in K.inputs(CASE, N).items()}
    sm = {k: v.to(DEV) for k, v in K.samples(CASE, N).items()}
    ret = K.returns_of(CASE, N).to(DEV)
    R, S = K.n_samples(CASE)
    out = header(n_random=R, n_next=S, critic_rows=N * (R + 3), target_rows=N * S, launches_per_call_read_off_the_code=84)
    eag, reps = timed(eager_step(b, sm, ret))
    out["eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
    print("eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        for draws in (False, True):
            ms, reps = timed(hip_step(make_model(prec), b, sm, ret, draws))
            out[f"{prec}{'/draws' if draws else ''}"] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
            print(prec, "draws" if draws else "given", ms, flush=True)
    write(path, out)


# ---- the actor arm ------------------------------------------------------------------------------------------------------------------
ACTOR_CASE = "kitchen_256"


def eager_actor_loss(actor, twin, obs, noise, alpha):
    """gaussian_calql.py:173-182 as plain torch (A.loss_actor without its diagnostics and host reads)."""
    s = A.sample(actor, ACTOR_CASE, obs, noise)
    q1, q2 = (A.q_forward(K.trunk(twin, i), ACTOR_CASE, obs, s["a"]) for i in (1, 2))
    return (-torch.min(q1, q2) + alpha * s["logp"]).mean()


def main_actor(path):
    b = {k: v.to(DEV) for k, v in A.inputs(ACTOR_CASE).items()}
    alpha = torch.full((1,), A.ALPHA, dtype=torch.float64, device=DEV)
    actor = {k: v.to(DEV).clone().requires_grad_(not k.startswith("logvar_m")) for k, v in A.actor_params(ACTOR_CASE).items()}
    twin = {k: v.to(DEV) for k, v in A.twin_params(ACTOR_CASE).items()}
    wrt = [v for v in actor.values() if v.requires_grad]
    L = len(K.CALQL_NETS[CASE][3])
    out = header(hidden_layers_per_trunk=L, launches_before_the_actors_backward_read_off_the_code=33)
    eag, reps = timed(lambda: torch.autograd.grad(eager_actor_loss(actor, twin, b["obs"], b["noise"], A.ALPHA), wrt))
    out["eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
    print("eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        m = make_model(prec)
        m.critic.load_state_dict(A.twin_params(ACTOR_CASE), strict=True)
        ms, reps = timed(lambda: m.loss_actor({"state": b["obs"]}, alpha, noise=b["noise"]))
        out[prec] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
        print(prec, ms, flush=True)
    write(path, out)


# ---- the iteration arm --------------------------------------------------------------------------------------------------------------
SEQ_LR, SEQ_ACTOR_LR, TAU = 3e-4, 1e-4, 0.005  # the shipped kitchen cfg's


def hip_iteration(prec, batch):
    from dppo_amd.agent.finetune.train_calql_agent import TrainCalQLAgent
    from dppo_amd.util.optim import FlatAdamW
    m = make_model(prec)
    agent = object.__new__(TrainCalQLAgent)  # update_iteration reads these and nothing else
    agent.model, agent.gamma, agent.target_ema_rate, agent.automatic_entropy_tuning, agent.target_entropy = m, K.GAMMA, TAU, True, -9.0
    agent.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=SEQ_LR, weight_decay=0)
    agent.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=SEQ_ACTOR_LR, weight_decay=0)
    agent.log_alpha = torch.zeros((), dtype=torch.float64, device=DEV, requires_grad=True)
    agent.log_alpha_optimizer = torch.optim.Adam([agent.log_alpha], lr=SEQ_LR)
    return lambda: agent.update_iteration(batches=batch)


def eager_iteration(batch):
    R, S = K.n_samples(CASE)
    od, ta, da = K.shapes(CASE)
    q = {k: v.to(DEV).clone().requires_grad_(True) for k, v in K.twin_params(CASE).items()}
    tq = {k: v.to(DEV).clone() for k, v in K.twin_params(CASE, K.TARGET_EPS).items()}
    actor = {k: v.to(DEV).clone().requires_grad_(not k.startswith("logvar_m")) for k, v in K.actor_params(CASE).items()}
    wrt = [v for v in actor.values() if v.requires_grad]
    la = torch.zeros((), dtype=torch.float64, device=DEV, requires_grad=True)
    opt_c = torch.optim.AdamW(list(q.values()), lr=SEQ_LR, weight_decay=0)
    opt_a = torch.optim.AdamW(wrt, lr=SEQ_ACTOR_LR, weight_decay=0)
    opt_t = torch.optim.Adam([la], lr=SEQ_LR)
    b = dict(obs=batch["obs"].reshape(N, 1, od), next_obs=batch["next_obs"].reshape(N, 1, od), actions=batch["actions"].reshape(N, ta, da),
             reward=batch["reward"], terminated=batch["terminated"])
    cur, nxt = batch["obs"], batch["next_obs"]

    def draw(n):
        return torch.randn(n, ta, da, device=DEV).clamp_(-A.RANDN_CLIP, A.RANDN_CLIP)

    def step():
        alpha = la.detach().exp().float()
        with torch.no_grad():  # the three policy samples of the critic loss, one stacked forward (the model's call order)
            s = A.sample({k: v.detach() for k, v in actor.items()}, ACTOR_CASE, torch.cat([nxt.repeat_interleave(S, dim=0), cur, nxt]),
                         draw(N * (S + 2)))
        a, lp = s["a"], s["logp"]
        sm = dict(next_actions=a[:N * S], pi_actions=a[N * S:N * S + N], log_pi=lp[N * S:N * S + N], pi_next_actions=a[N * S + N:],
                  log_pi_next=lp[N * S + N:])
        bb = dict(b, random_actions=torch.rand(N, R, ta, da, device=DEV) * 2 - 1)
        rc = K.loss_critic(q, tq, CASE, bb, sm, batch["returns"], host_stats=False)
        for t, g in zip(q.values(), rc["grads"]):
            t.grad = g
        opt_c.step()
        with torch.no_grad():
            torch._foreach_lerp_(list(tq.values()), [v.detach() for v in q.values()], TAU)
        stepped = {k: v.detach() for k, v in q.items()}
        for t, g in zip(wrt, torch.autograd.grad(eager_actor_loss(actor, stepped, cur, draw(N), alpha), wrt)):
            t.grad = g
        opt_a.step()
        with torch.no_grad():
            logp = A.sample({k: v.detach() for k, v in actor.items()}, ACTOR_CASE, cur, draw(N))["logp"]
        opt_t.zero_grad()
        (-torch.mean(la.exp() * (logp + (-9.0)))).backward()
        opt_t.step()
    return step


def main_iteration(path):
    b = {k: v.to(DEV) for k, v in K.inputs(CASE, N).items()}
    batch = dict(obs=b["obs"].reshape(N, -1), next_obs=b["next_obs"].reshape(N, -1), actions=b["actions"].reshape(N, -1),
                 reward=b["reward"], terminated=b["terminated"], returns=K.returns_of(CASE, N).to(DEV))
    out = header(steps="policy samples and random actions drawn, critic loss + AdamW + Polyak, actor loss + AdamW, temperature loss + Adam",
                 launches_read_off_the_code=dict(critic_loss=84, actor_loss_before_the_actors_backward=33))
    eag, reps = timed(eager_iteration(batch))
    out["eager_torch_fp32"] = dict(ms_per_update=eag, updates_per_pass=reps)
    print("eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        ms, reps = timed(hip_iteration(prec, batch))
        out[prec] = dict(ms_per_update=ms, updates_per_pass=reps, eager_over_hip=eag / ms)
        print(prec, ms, flush=True)
    write(path, out)


if __name__ == "__main__":
    arms = {"critic": main, "actor": main_actor, "iteration": main_iteration}
    arm, path = (sys.argv[1], sys.argv[2]) if len(sys.argv) > 2 else ("critic", sys.argv[1])
    arms[arm](path)
