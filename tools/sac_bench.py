"""Time SAC's update at the shipped halfcheetah shape (batch 256, hidden [256, 256], Ta*Da = 6), bf16 and fp32:

    python3 tools/sac_bench.py profiles/sac_update.json

  update  one TrainSACAgent.update_minibatch out of a full replay ring: the temperature's snapshot, critic TD loss (with the sample
          at the next observations) + step, Polyak, then twice: actor loss + step, temperature loss + step;
  eager   the same update as plain torch on the same GPU: tests/golden/make_golden_sac_cases.py's restatement (the reference's
          arithmetic) under autograd with torch.optim.Adam, fp32, draws from torch.randn, alpha read back once per update with
          ``.item()`` as the reference agent does.
Every arm is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported
(tools/idql_bench.timed).  First measurements of a new path: no threshold is set."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.idql_bench import measured_on, timed  # noqa: E402

CFG = "gym/scratch/halfcheetah-v2/sac_mlp.yaml"


def make_agent(prec, logdir):
    import copy
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    from dppo_amd.cfg.loader import Cfg, load_config
    cfg = copy.deepcopy(load_config(os.path.join(ROOT, "tests", "golden", "shipped_sac_cfgs.json"))[CFG])
    cfg.update(device="cuda:0", seed=0, logdir=logdir, env=Cfg(n_envs=8, name="synthetic", max_episode_steps=100))
    cfg.pop("wandb", None)
    cfg.model.update(device="cuda:0")
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = prec
    cfg.train.update(buffer_size=64)
    agent = TrainSACAgent(cfg)
    rp = agent.replay
    for t in (rp.obs, rp.next_obs, rp.actions):
        t.uniform_(-1, 1)
    rp.reward.uniform_(0, 4)
    rp.terminated.bernoulli_(0.05)
    rp.steps, rp.head = rp.cap, 7
    return agent


def eager_update(agent):
    """The restatement as an eager torch update on the agent's device, with its own copies of the weights."""
    from tests.golden import make_golden_sac_cases as K
    dev, case = agent.device, "cheetah"
    leaf = lambda sd: {k: v.detach().clone().to(dev).requires_grad_(not k.startswith("logvar_m")) for k, v in sd.items()}
    a, q = leaf(agent.model.network.state_dict()), leaf(agent.model.critic.state_dict())
    tq = {k: v.detach().clone() for k, v in q.items()}
    la = torch.zeros((), dtype=torch.float64, device=dev, requires_grad=True)
    opt_a = torch.optim.Adam([v for v in a.values() if v.requires_grad], lr=3e-4)
    opt_c, opt_t = torch.optim.Adam(list(q.values()), lr=1e-3), torch.optim.Adam([la], lr=1e-3)
    rp, N, te = agent.replay, agent.batch_size, K.target_entropy(case)
    z = lambda: torch.randn(N, 6, device=dev)

    def step(inds):
        obs, nxt, act, rew, term = rp.gather(inds)
        alpha = la.exp().item()
        with torch.no_grad():
            s = K.sample(a, case, nxt, z())
            y = rew + K.GAMMA * (torch.min(*K.twin_forward(tq, case, nxt, s["a"])) - alpha * s["logp"]) * (1 - term)
        q1, q2 = K.twin_forward(q, case, obs, act)
        loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
        opt_c.zero_grad()
        loss.backward()
        opt_c.step()
        with torch.no_grad():
            for k in tq:
                tq[k].copy_(tq[k] * (1.0 - 0.005) + q[k] * 0.005)
        for _ in range(2):
            s = K.sample(a, case, obs, z())
            la_loss = (-torch.min(*K.twin_forward(q, case, obs, s["a"])) + alpha * s["logp"]).mean()
            opt_a.zero_grad()
            la_loss.backward()
            opt_a.step()
            with torch.no_grad():
                lp = K.sample(a, case, obs, z())["logp"]
            lt = -torch.mean(la.exp() * (lp + te))
            opt_t.zero_grad()
            lt.backward()
            opt_t.step()
    return step


def main(path):
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(),
               method="median of 10 passes of >= 0.5 s between device events, every arm warmed")
    with tempfile.TemporaryDirectory() as logdir:
        for prec in ("bf16", "fp32"):
            agent = make_agent(prec, logdir)
            inds = agent.replay.draw(64, agent.batch_size)
            it = iter(range(10 ** 9))
            upd, reps = timed(lambda: agent.update_minibatch(inds[next(it) % 64]))
            out[f"cheetah/{prec}"] = dict(batch=agent.batch_size, ms_per_update=upd, updates_per_pass=reps)
            print(prec, out[f"cheetah/{prec}"], flush=True)
        step = eager_update(agent)
        eag, reps = timed(lambda: step(inds[next(it) % 64]))
        out["cheetah/eager_torch_fp32"] = dict(batch=agent.batch_size, ms_per_update=eag, updates_per_pass=reps)
        for prec in ("bf16", "fp32"):
            out[f"cheetah/{prec}"]["eager_over_hip"] = eag / out[f"cheetah/{prec}"]["ms_per_update"]
        print(out, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
