"""Time IBRL's model at the shipped can shape (obs 23, Ta*Da = 7, actor and members 3 x 1024 ReLU, E = 5, dropout 0.5), bf16 and fp32:

    python3 tools/ibrl_bench.py profiles/ibrl_model.json [forward,loss_critic]
    python3 tools/ibrl_bench.py profiles/ibrl_actor.json actor
    python3 tools/ibrl_bench.py profiles/ibrl_iteration.json iteration

  forward      IBRL_Gaussian.forward (dppo_ibrl_act: both actors with dropout live, the pair's two members over 2B rows, the soft
               choice) at B = 1 -- the shipped cfgs' n_envs: 1, n_steps: 1, so every training iteration is one such call -- and at
               B = 256; every draw (noise, masks, u, the pair) is made per call, as the agent would;
  loss_critic  IBRL_Gaussian.loss_critic at batch 256 out of plain tensors: the two next-action samples (two dppo_gaussian_sample_drop
               calls) and dppo_ibrl_q_loss_fwd_bwd; the gradient is left in critic_flat_grads(); no optimiser step on either side;
  actor        IBRL_Gaussian.loss_actor at batch 256 out of plain tensors (dppo_ibrl_actor_fwd_bwd: the actor's forward with dropout,
               all E members' forwards and chains, the actor's backward); noise and mask are drawn per call; no optimiser step;
  iteration    TrainIBRLAgent.update_iteration's work at the shipped critic_num_update = 3: three times [batch indices drawn on the
               host, loss_critic off the ring, FlatAdamW step, Polyak], one loss_actor off the ring, its step, the target actor's
               Polyak; the eager side does the same with torch.optim.AdamW(foreach) and a lerp per target tensor;
  eager        the restatement of tests/golden/make_golden_ibrl_cases.py (fp32) as plain torch on the same GPU, its masks, noise and
               u drawn by torch per call, and for the loss torch.autograd.grad over all members' parameters.
Every arm is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported
(tools/idql_bench.timed).  The launch counts are csrc/ibrl.h's (read off the code).  First measurements of a new path: no threshold
is set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.golden import make_golden_ibrl_cases as K  # noqa: E402
from tools.idql_bench import measured_on, timed  # noqa: E402

DEV, CASE, N = "cuda:0", "can", 256
METHOD = "median of 10 passes of >= 0.5 s between device events, every arm warmed"


def make_model(prec):
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_ibrl import IBRL_Gaussian
    od, ta, da, dims, act, p, qdims, qact, E = K.IBRL_NETS[CASE]
    actor = Gaussian_MLP(da, ta, od, mlp_dims=list(dims), activation_type=act, dropout=p, fixed_std=K.FIXED_STD, precision=prec,
                         plain_fixed_std=True)
    critic = CriticObsAct(cond_dim=od, mlp_dims=list(qdims), action_dim=da, action_steps=ta, activation_type=qact, use_layernorm=True,
                          double_q=False, precision=prec)
    m = IBRL_Gaussian(actor=actor, critic=critic, n_critics=E, soft_action_sample=True, soft_action_sample_beta=K.BETA, horizon_steps=ta,
                      device=DEV, randn_clip_value=K.RANDN_CLIP)
    for name, net in (("bc", m.bc_policy), ("rl", m.network), ("target", m.target_actor)):
        net.load_state_dict(K.actor_state_dict(CASE, name), strict=True)
    for e in range(E):
        m.critic_networks[e].load_state_dict(K.member_params(CASE, e), strict=True)
        m.target_networks[e].load_state_dict(K.member_params(CASE, e, K.TARGET_EPS), strict=True)
    return m


def on_dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def draws(n):
    od, ta, da, dims = K.IBRL_NETS[CASE][:4]
    mask = lambda: (torch.rand(len(dims), n, dims[0], device=DEV) >= K.dropout(CASE)).to(torch.uint8)
    return mask(), torch.randn(n, ta * da, device=DEV), mask(), torch.randn(n, ta * da, device=DEV)


def eager_forward(obs):
    """gaussian_ibrl.py:149-205 with torch's own draws; the reference's softmax and multinomial."""
    bc, rl = on_dev(K.actor_params(CASE, "bc")), on_dev(K.actor_params(CASE, "rl"))
    members = [on_dev(K.member_params(CASE, e)) for e in range(K.n_critics(CASE))]
    n = len(obs)

    def step():
        with torch.no_grad():
            i, j = torch.randperm(len(members))[:2].tolist()
            mb, zb, mr, zr = draws(n)
            a_bc, _ = K.sample(bc, CASE, obs, mb, zb, K.BC_STD)
            a_rl, _ = K.sample(rl, CASE, obs, mr, zr, K.FIXED_STD)
            q_bc = torch.min(K.q_forward(members[i], CASE, obs, a_bc), K.q_forward(members[j], CASE, obs, a_bc))
            q_rl = torch.min(K.q_forward(members[i], CASE, obs, a_rl), K.q_forward(members[j], CASE, obs, a_rl))
            w = torch.softmax(torch.stack([torch.exp(q_bc * K.BETA), torch.exp(q_rl * K.BETA)], dim=-1), dim=-1)
            w = torch.where(torch.isnan(w), torch.full_like(w, 0.5), w)  # (the overflow row: multinomial would raise)
            return torch.where(torch.multinomial(w, 1) == 0, a_bc, a_rl)
    return step


def eager_critic(b):
    E = K.n_critics(CASE)
    members = [{k: v.to(DEV).clone().requires_grad_(True) for k, v in K.member_params(CASE, e).items()} for e in range(E)]
    targets = [on_dev(K.member_params(CASE, e, K.TARGET_EPS)) for e in range(E)]
    bc, tg = on_dev(K.actor_params(CASE, "bc")), on_dev(K.actor_params(CASE, "target"))
    flat = [t for p in members for t in p.values()]

    def step():
        i, j = torch.randperm(E)[:2].tolist()
        with torch.no_grad():
            mb, zb, mr, zr = draws(N)
            a_bc, _ = K.sample(bc, CASE, b["next_obs"], mb, zb, K.BC_STD)
            a_rl, _ = K.sample(tg, CASE, b["next_obs"], mr, zr, K.FIXED_STD)
            qb = torch.min(K.q_forward(targets[i], CASE, b["next_obs"], a_bc), K.q_forward(targets[j], CASE, b["next_obs"], a_bc))
            qr = torch.min(K.q_forward(targets[i], CASE, b["next_obs"], a_rl), K.q_forward(targets[j], CASE, b["next_obs"], a_rl))
            y = b["reward"] + K.GAMMA * (1 - b["terminated"]) * torch.where(qb > qr, qb, qr)
        q = torch.stack([K.q_forward(p, CASE, b["obs"], b["actions"]) for p in members])
        return torch.autograd.grad(torch.mean((q - y[None]) ** 2), flat)
    return step


def eager_actor(b, members=None, actor=None):
    """gaussian_ibrl.py:115-128 with torch's own draws."""
    from tests.golden import make_golden_ibrl_actor_cases as A
    E = K.n_critics(CASE)
    members = members if members is not None else [on_dev(K.member_params(CASE, e)) for e in range(E)]
    actor = actor if actor is not None else {k: v.to(DEV).clone().requires_grad_(True) for k, v in K.actor_params(CASE, "rl").items()}
    flat = list(actor.values())

    def step():
        mask, z, _, _ = draws(N)
        loc = torch.tanh(A.actor_pre(actor, CASE, b["obs"], mask))
        scale = torch.ones_like(loc) * K.FIXED_STD
        a = torch.clamp(loc + z * scale, loc - K.RANDN_CLIP * scale, loc + K.RANDN_CLIP * scale)
        q = torch.stack([K.q_forward({k: v.detach() for k, v in p.items()}, CASE, b["obs"], a) for p in members])
        return torch.autograd.grad(-torch.mean(q.min(dim=0).values), flat)
    return step


def eager_iteration(b, k_updates, lr=1e-4, tau=0.01):
    E = K.n_critics(CASE)
    members = [{k: v.to(DEV).clone().requires_grad_(True) for k, v in K.member_params(CASE, e).items()} for e in range(E)]
    targets = [on_dev(K.member_params(CASE, e, K.TARGET_EPS)) for e in range(E)]
    actor = {k: v.to(DEV).clone().requires_grad_(True) for k, v in K.actor_params(CASE, "rl").items()}
    bc, tg = on_dev(K.actor_params(CASE, "bc")), on_dev(K.actor_params(CASE, "target"))
    flat = [t for p in members for t in p.values()]
    tflat = [t for p in targets for t in p.values()]
    opt_c, opt_a = torch.optim.AdamW(flat, lr=lr, weight_decay=0), torch.optim.AdamW(list(actor.values()), lr=lr, weight_decay=0)
    ring = {k: b[k] for k in ("obs", "next_obs", "actions", "reward", "terminated")}

    def step():
        for _ in range(k_updates):
            inds = torch.from_numpy(np.random.choice(N, N)).to(DEV)
            mb = {k: v[inds] for k, v in ring.items()}
            i, j = torch.randperm(E)[:2].tolist()
            with torch.no_grad():
                m1, z1, m2, z2 = draws(N)
                a_bc, _ = K.sample(bc, CASE, mb["next_obs"], m1, z1, K.BC_STD)
                a_rl, _ = K.sample(tg, CASE, mb["next_obs"], m2, z2, K.FIXED_STD)
                qb = torch.min(K.q_forward(targets[i], CASE, mb["next_obs"], a_bc), K.q_forward(targets[j], CASE, mb["next_obs"], a_bc))
                qr = torch.min(K.q_forward(targets[i], CASE, mb["next_obs"], a_rl), K.q_forward(targets[j], CASE, mb["next_obs"], a_rl))
                y = mb["reward"] + K.GAMMA * (1 - mb["terminated"]) * torch.where(qb > qr, qb, qr)
            q = torch.stack([K.q_forward(p, CASE, mb["obs"], mb["actions"]) for p in members])
            for t, g in zip(flat, torch.autograd.grad(torch.mean((q - y[None]) ** 2), flat)):
                t.grad = g
            opt_c.step()
            with torch.no_grad():
                torch._foreach_lerp_(tflat, [t.detach() for t in flat], tau)
        for t, g in zip(actor.values(), eager_actor(mb, members, actor)()):
            t.grad = g
        opt_a.step()
        with torch.no_grad():
            torch._foreach_lerp_(list(tg.values()), [t.detach() for t in actor.values()], tau)
    return step


def hip_iteration(m, b, k_updates, lr=1e-4, tau=0.01):
    from dppo_amd.util.optim import FlatAdamW
    from dppo_amd.util.replay import DeviceReplay
    od, ta, da = K.shapes(CASE)
    rp = DeviceReplay(N, 1, od, ta * da, DEV)
    rp.extend(b["obs"].reshape(N, 1, -1), b["next_obs"].reshape(N, 1, -1), b["actions"].reshape(N, 1, -1), b["reward"].reshape(N, 1),
              b["terminated"].reshape(N, 1))
    opt_c, opt_a = FlatAdamW(m.critic_flat_params(), lr=lr, weight_decay=0), FlatAdamW(m.network.flat_params(), lr=lr, weight_decay=0)
    m.train()

    def step():
        for _ in range(k_updates):
            inds = torch.from_numpy(np.random.choice(N, N).astype(np.int64)).to(DEV)
            m.loss_critic(rp, None, None, None, None, K.GAMMA, inds=inds)
            opt_c.step(m.critic_flat_grads())
            m.critics_updated()
            m.update_target_critic(tau)
        m.loss_actor(rp, inds)
        opt_a.step(m.last_loss_grad)
        m.network.mark_updated()
        m.update_target_actor(tau)
    return step


def new_arms(path, arms):
    """The actor loss and the whole iteration, each into a file of its own."""
    b = on_dev(K.inputs(CASE, N))
    b = {k: (v.reshape(N, -1) if v.dim() > 1 and k in ("obs", "next_obs", "actions") else v) for k, v in b.items()}
    L, E, k_updates = len(K.IBRL_NETS[CASE][3]), K.n_critics(CASE), 3
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(), method=METHOD,
               shape=dict(obs=23, act_flat=7, hidden=1024, hidden_layers=L, E=E, dropout=K.dropout(CASE), batch=N,
                          critic_num_update=k_updates),
               launches_read_off_the_code=dict(actor_before_the_actors_backward=2 + (2 * L + 1) + 1 + E * (2 * L + 1) + 1 + E * (2 * L - 1) + 2))
    for arm in arms:
        eag, reps = timed(eager_actor(b) if arm == "actor" else eager_iteration(b, k_updates))
        out[f"{arm}/eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
        print(arm, "eager", eag, flush=True)
        for prec in ("bf16", "fp32"):
            m = make_model(prec)
            m.train()
            step = (lambda: m.loss_actor({"state": b["obs"]})) if arm == "actor" else hip_iteration(m, b, k_updates)
            ms, reps = timed(step)
            out[f"{arm}/{prec}"] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
            print(arm, prec, ms, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main(path):
    b = on_dev(K.inputs(CASE, N))
    fb = on_dev(K.forward_inputs(CASE, N))
    L = len(K.IBRL_NETS[CASE][3])
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(), method=METHOD,
               shape=dict(obs=23, act_flat=7, hidden=1024, hidden_layers=L, E=K.n_critics(CASE), dropout=K.dropout(CASE), batch=N),
               launches_read_off_the_code=dict(forward=33, loss_critic_before_the_members_backwards=1 + 7 * (2 + K.n_critics(CASE)) + 5,
                                               next_action_samples=2 * 9))
    for B in (1, N):
        obs = fb["obs"][:B].contiguous()
        eag, reps = timed(eager_forward(obs))
        out[f"forward_B{B}/eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
        print("forward", B, "eager", eag, flush=True)
        for prec in ("bf16", "fp32"):
            m = make_model(prec)
            ms, reps = timed(lambda: m({"state": obs}))
            out[f"forward_B{B}/{prec}"] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
            print("forward", B, prec, ms, flush=True)
    eag, reps = timed(eager_critic(b))
    out["loss_critic/eager_torch_fp32"] = dict(ms_per_call=eag, calls_per_pass=reps)
    print("loss_critic eager", eag, flush=True)
    for prec in ("bf16", "fp32"):
        m = make_model(prec)
        step = lambda: m.loss_critic({"state": b["obs"]}, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA)
        ms, reps = timed(step)
        out[f"loss_critic/{prec}"] = dict(ms_per_call=ms, calls_per_pass=reps, eager_over_hip=eag / ms)
        print("loss_critic", prec, ms, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    picked = [a for a in (sys.argv[2].split(",") if len(sys.argv) > 2 else []) if a in ("actor", "iteration")]
    if picked:
        new_arms(sys.argv[1], picked)
    else:
        main(sys.argv[1])
