"""Time DQL's update at the shipped hopper and can shapes, bf16 and fp32:

    python3 tools/dql_bench.py profiles/dql_update.json

  update      one minibatch of TrainDQLDiffusionAgent.update_minibatch at batch 1000 out of a full replay ring: critic TD loss (with
              the K-step sampler call that draws a' at the next observations) + step, loss_actor + step, Polyak;
  loss_actor  DQLDiffusion.loss_actor alone: the sampler call that writes the chain, then dppo_dql_actor_fwd_bwd;
  sampler     that sampler call alone (forward_train with every chain position kept).
The timing method is tools/qsm_bench.py's (every shape warmed, each pass >= 0.5 s of work between two device events, the median of
ten passes).  First measurements of a new path: nothing to compare them with, no threshold.  The launch count of loss_actor comes
from profiler runs of their own (never timed under the profiler), at the cfg's K and at half of it -- the check that the
weight-gradient launches do not grow with K (what grows is the per-slab chain: its GEMMs and one link per step):

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 tools/dql_bench.py --trace hopper bf16 20
    python3 tools/dql_bench.py profiles/dql_update.json --launches out/<host>/<pid>_kernel_stats.csv hopper bf16 20
"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.idql_bench import TRACE_STEPS, TRACE_WARM, measured_on, timed  # noqa: E402
from tools.qsm_bench import count_launches  # noqa: E402

SHAPES = {"hopper": dict(cfg="gym/finetune/hopper-v2/ft_dql_diffusion_mlp.yaml", B=40),
          "can": dict(cfg="robomimic/finetune/can/ft_dql_diffusion_mlp.yaml", B=50)}


def make_agent(shape, prec, logdir, steps=None):
    import copy
    from dppo_amd.agent.finetune.train_dql_diffusion_agent import TrainDQLDiffusionAgent
    from dppo_amd.cfg.loader import Cfg, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = copy.deepcopy(load_config(os.path.join(root, "tests", "golden", "shipped_dql_cfgs.json"))[SHAPES[shape]["cfg"]])
    cfg.update(device="cuda:0", seed=0, logdir=logdir, env=Cfg(n_envs=SHAPES[shape]["B"], name="synthetic", max_episode_steps=100))
    cfg.pop("wandb", None)
    cfg.model.update(device="cuda:0", network_path=None)
    if steps is not None:
        cfg.model.update(denoising_steps=int(steps))
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = prec
    cfg.train.update(buffer_size=64, n_critic_warmup_itr=0)
    agent = TrainDQLDiffusionAgent(cfg)
    rp = agent.replay
    for t in (rp.obs, rp.next_obs, rp.actions):
        t.uniform_(-1, 1)
    rp.reward.uniform_(0, 0.04)
    rp.terminated.bernoulli_(0.05)
    rp.steps, rp.head = rp.cap, 7
    return agent


def main():
    args = sys.argv[1:]
    with tempfile.TemporaryDirectory() as logdir:
        if args[0] == "--trace":
            agent = make_agent(args[1], args[2], logdir, args[3] if len(args) > 3 else None)
            inds = agent.replay.draw(TRACE_WARM + TRACE_STEPS, agent.batch_size)
            for b in range(TRACE_WARM + TRACE_STEPS):
                agent.model.loss_actor(agent.replay, agent.eta, agent.act_steps, inds=inds[b])
            torch.cuda.synchronize()
            return
        path = args[0]
        out = json.load(open(path)) if os.path.exists(path) else {}
        if len(args) > 1 and args[1] == "--launches":
            c = count_launches(args[2], TRACE_WARM + TRACE_STEPS)
            out.setdefault(f"{args[3]}/{args[4]}", {}).update({f"launches_per_loss_actor_K{args[5]}": c["launches"],
                                                              f"kernels_by_calls_per_loss_actor_K{args[5]}": c["kernels_by_calls"]})
        else:
            out.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(),
                       method="median of 10 passes of >= 0.5 s between device events, every shape warmed")
            for shape in SHAPES:
                for prec in ("bf16", "fp32"):
                    agent = make_agent(shape, prec, logdir)
                    m = agent.model
                    inds = agent.replay.draw(64, agent.batch_size)
                    it = iter(range(10 ** 9))
                    upd, reps_u = timed(lambda: agent.update_minibatch(inds[next(it) % 64]))
                    act, reps_a = timed(lambda: m.loss_actor(agent.replay, agent.eta, agent.act_steps, inds=inds[0]))
                    st = agent.replay.gather(inds[0])[0]
                    smp, _ = timed(lambda: m.forward_train({"state": st}, return_chain=True))
                    out.setdefault(f"{shape}/{prec}", {}).update(batch=agent.batch_size, denoising_steps=m.denoising_steps,
                                                                 ms_per_update=upd, updates_per_pass=reps_u, ms_per_loss_actor=act,
                                                                 loss_actors_per_pass=reps_a, ms_per_chain_sampler_call=smp)
                    print(shape, prec, out[f"{shape}/{prec}"], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
