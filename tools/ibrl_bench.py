"""Time IBRL's model at the shipped can shape (obs 23, Ta*Da = 7, actor and members 3 x 1024 ReLU, E = 5, dropout 0.5), bf16 and fp32:

    python3 tools/ibrl_bench.py profiles/ibrl_model.json

  forward      IBRL_Gaussian.forward (dppo_ibrl_act: both actors with dropout live, the pair's two members over 2B rows, the soft
               choice) at B = 1 -- the shipped cfgs' n_envs: 1, n_steps: 1, so every training iteration is one such call -- and at
               B = 256; every draw (noise, masks, u, the pair) is made per call, as the agent would;
  loss_critic  IBRL_Gaussian.loss_critic at batch 256 out of plain tensors: the two next-action samples (two dppo_gaussian_sample_drop
               calls) and dppo_ibrl_q_loss_fwd_bwd; the gradient is left in critic_flat_grads(); no optimiser step on either side;
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
    main(sys.argv[1])
