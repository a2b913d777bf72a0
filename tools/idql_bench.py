"""Time IDQL's two hot loops at the shipped hopper and can shapes, bf16 and fp32:

    python3 tools/idql_bench.py profiles/idql_update.json

  update   one minibatch of TrainIDQLDiffusionAgent.update_minibatch at batch 1000: V loss + step, Q loss + step, Polyak +
           re-pack, actor MSE + step, out of a full replay ring;
  forward  one IDQLDiffusion.forward (K = 20 denoising steps, target twin, V, selection) at B * S = 40 * 20 / 50 * 10.
Every shape is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported.
Launches per update come from a profiler run of their own (never timed under the profiler):

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 tools/idql_bench.py --trace hopper bf16
    python3 tools/idql_bench.py profiles/idql_update.json --launches out/<host>/<pid>_kernel_stats.csv hopper bf16

``--trace`` runs 10 warm-up and 100 counted updates and nothing else; ``--launches`` counts the kernels
launched at least once per update (110 calls or more), the runtime's copy kernels apart, divides by 110 and stores the result
beside that shape's timing."""
import csv
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def measured_on():
    """The accelerator the numbers were taken on, from the device itself: its gfx architecture, and the product it is."""
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    return {"gfx950": "MI355X (gfx950)"}.get(arch, arch)

SHAPES = {"hopper": dict(cfg="gym/finetune/hopper-v2/ft_idql_diffusion_mlp.yaml", B=40, S=20),
          "can": dict(cfg="robomimic/finetune/can/ft_idql_diffusion_mlp.yaml", B=50, S=10)}
TRACE_WARM, TRACE_STEPS = 10, 100


def make_agent(shape, prec, logdir):
    import copy
    from dppo_amd.agent.finetune.train_idql_diffusion_agent import TrainIDQLDiffusionAgent
    from dppo_amd.cfg.loader import Cfg, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = copy.deepcopy(load_config(os.path.join(root, "tests", "golden", "shipped_idql_cfgs.json"))[SHAPES[shape]["cfg"]])
    cfg.update(device="cuda:0", seed=0, logdir=logdir, env=Cfg(n_envs=SHAPES[shape]["B"], name="synthetic", max_episode_steps=100))
    cfg.pop("wandb", None)
    cfg.model.update(device="cuda:0", network_path=None)
    for node in (cfg.model.actor, cfg.model.critic_q, cfg.model.critic_v):
        node["precision"] = prec
    cfg.train.update(buffer_size=64, n_critic_warmup_itr=0)
    agent = TrainIDQLDiffusionAgent(cfg)
    rp = agent.replay
    for t in (rp.obs, rp.next_obs, rp.actions):
        t.uniform_(-1, 1)
    rp.reward.uniform_(0, 0.04)
    rp.terminated.bernoulli_(0.05)
    rp.steps, rp.head = rp.cap, 7
    return agent


def timed(fn, min_ms=500.0, passes=10):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, out = 8, []
    while len(out) < passes:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms < min_ms:  # not enough work between the events yet: grow the pass, do not count it
            reps = int(reps * max(2.0, 1.2 * min_ms / max(ms, 1e-3)))
            continue
        out.append(ms / reps)
    return statistics.median(out), reps


def main():
    args = sys.argv[1:]
    with tempfile.TemporaryDirectory() as logdir:
        if args[0] == "--trace":
            agent = make_agent(args[1], args[2], logdir)
            inds = agent.replay.draw(TRACE_WARM + TRACE_STEPS, agent.batch_size)
            for b in range(TRACE_WARM + TRACE_STEPS):
                agent.update_minibatch(inds[b])
            torch.cuda.synchronize()
            return
        path = args[0]
        out = json.load(open(path)) if os.path.exists(path) else {}
        if len(args) > 1 and args[1] == "--launches":
            rows = list(csv.DictReader(open(args[2])))
            n = TRACE_WARM + TRACE_STEPS
            # a kernel of the update is launched at least once per update; rows with fewer calls than updates belong to the
            # agent's construction.  The runtime's own copy kernels (device-to-device copies torch queues: clones, the
            # gathered rows of the actor's batch) are counted apart from the project's kernels.
            per = [r for r in rows if int(r["Calls"]) >= n]
            rt = [r for r in per if r["Name"].startswith("__amd_rocclr")]
            own = [r for r in per if not r["Name"].startswith("__amd_rocclr")]
            key = f"{args[3]}/{args[4]}"
            out.setdefault(key, {}).update(launches_per_update=sum(int(r["Calls"]) for r in own) / n,
                                           runtime_copy_launches_per_update=sum(int(r["Calls"]) for r in rt) / n,
                                           one_off_launches=sum(int(r["Calls"]) for r in rows if int(r["Calls"]) < n),
                                           kernels_by_calls_per_update={r["Name"][:60]: int(r["Calls"]) / n for r in per})
        else:
            out.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(),
                       method="median of 10 passes of >= 0.5 s between device events, every shape warmed")
            for shape in SHAPES:
                for prec in ("bf16", "fp32"):
                    agent = make_agent(shape, prec, logdir)
                    inds = agent.replay.draw(64, agent.batch_size)
                    it = iter(range(10 ** 9))
                    upd, reps_u = timed(lambda: agent.update_minibatch(inds[next(it) % 64]))
                    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
                    state = torch.rand(B, agent.n_cond_step, agent.obs_dim, device="cuda:0") * 2 - 1
                    fwd, reps_f = timed(lambda: agent.model(cond={"state": state}, num_sample=S))
                    det, _ = timed(lambda: agent.model(cond={"state": state}, num_sample=S, deterministic=True))
                    out.setdefault(f"{shape}/{prec}", {}).update(batch=agent.batch_size, ms_per_update=upd, updates_per_pass=reps_u,
                                                                 forward_rows=B * S, ms_per_forward=fwd, ms_per_forward_argmax=det,
                                                                 forwards_per_pass=reps_f)
                    print(shape, prec, out[f"{shape}/{prec}"], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
