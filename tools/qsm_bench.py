"""Time QSM's update at the shipped hopper and can shapes, bf16 and fp32:

    python3 tools/qsm_bench.py profiles/qsm_update.json

  update   one minibatch of TrainQSMDiffusionAgent.update_minibatch at batch 1000 out of a full replay ring: critic TD loss (with
           the K-step sampler call that draws a' at the 1000 next observations) + step, the actor target + denoising MSE + step,
           Polyak;
  sampler  that sampler call alone (QSMDiffusion.forward on 1000 rows), the part of the update no other baseline here has;
  target   dppo_qsm_actor_target alone (the critic's action gradient: row builder, two forwards, two data-gradient chains, tail).
Every shape is warmed, each pass times >= 0.5 s of work between two device events, the median of ten passes is reported.  These
are first measurements of a new path: there is nothing to compare them with, and no threshold.  Launches per update come from a
profiler run of their own (never timed under the profiler):

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 tools/qsm_bench.py --trace hopper bf16
    python3 tools/qsm_bench.py profiles/qsm_update.json --launches out/<host>/<pid>_kernel_stats.csv hopper bf16

``--trace`` runs 10 warm-up and 100 counted updates and nothing else (``--trace-target``: the same for the actor-target call
alone); ``--launches`` (``--launches-target``) counts the kernels launched at least once per update (110 calls or more), the
runtime's copy kernels apart, divides by 110 and stores the result beside that shape's timing."""
import csv
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.idql_bench import TRACE_STEPS, TRACE_WARM, measured_on, timed  # noqa: E402

SHAPES = {"hopper": dict(cfg="gym/finetune/hopper-v2/ft_qsm_diffusion_mlp.yaml", B=40),
          "can": dict(cfg="robomimic/finetune/can/ft_qsm_diffusion_mlp.yaml", B=50)}


def make_agent(shape, prec, logdir):
    import copy
    from dppo_amd.agent.finetune.train_qsm_diffusion_agent import TrainQSMDiffusionAgent
    from dppo_amd.cfg.loader import Cfg, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = copy.deepcopy(load_config(os.path.join(root, "tests", "golden", "shipped_qsm_cfgs.json"))[SHAPES[shape]["cfg"]])
    cfg.update(device="cuda:0", seed=0, logdir=logdir, env=Cfg(n_envs=SHAPES[shape]["B"], name="synthetic", max_episode_steps=100))
    cfg.pop("wandb", None)
    cfg.model.update(device="cuda:0", network_path=None)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = prec
    cfg.train.update(buffer_size=64, n_critic_warmup_itr=0)
    agent = TrainQSMDiffusionAgent(cfg)
    rp = agent.replay
    for t in (rp.obs, rp.next_obs, rp.actions):
        t.uniform_(-1, 1)
    rp.reward.uniform_(0, 0.04)
    rp.terminated.bernoulli_(0.05)
    rp.steps, rp.head = rp.cap, 7
    return agent


def target_only(agent, inds):
    """The library call of loss_actor without the denoising MSE behind it."""
    import ctypes as C
    from dppo_amd import hip
    m = agent.model
    q, N = m.critic_q, inds.numel()
    lib, dq, dev = hip.load(), q.net_desc(), inds.device
    AF, OD = m.horizon_steps * m.action_dim, q.cond_dim
    ws = m._ws_target.get(lib.dppo_qsm_actor_target_workspace_bytes(C.byref(dq), m.prec, OD, N), dev)
    k1, k2 = q.packed(m.prec)
    sa, sb = m._tables(dev)
    noise, t = torch.randn(N, AF, device=dev), torch.randint(0, m.denoising_steps, (N,), device=dev)
    pairs, obs_out = torch.empty(N, 2, AF, device=dev), torch.empty(N, OD, device=dev)
    batch = agent.replay.batch(inds)

    def call():
        hip.check(lib.dppo_qsm_actor_target(
            C.byref(dq), m.prec, q.flat_params().data_ptr(), k1.data_ptr(), k2.data_ptr(), C.byref(batch), OD, N, noise.data_ptr(),
            t.data_ptr(), sa.data_ptr(), sb.data_ptr(), m.denoising_steps, float(agent.q_grad_coeff), pairs.data_ptr(),
            obs_out.data_ptr(), None, ws.data_ptr(), ws.numel(), hip.stream()), "dppo_qsm_actor_target")
    return call


def count_launches(path, n):
    rows = list(csv.DictReader(open(path)))
    # a kernel of the update is launched at least once per update; rows with fewer calls than updates belong to the agent's
    # construction.  The runtime's own copy kernels (device-to-device copies torch queues) are counted apart.
    per = [r for r in rows if int(r["Calls"]) >= n]
    rt = [r for r in per if r["Name"].startswith("__amd_rocclr")]
    own = [r for r in per if not r["Name"].startswith("__amd_rocclr")]
    return dict(launches=sum(int(r["Calls"]) for r in own) / n, runtime_copy_launches=sum(int(r["Calls"]) for r in rt) / n,
                one_off_launches=sum(int(r["Calls"]) for r in rows if int(r["Calls"]) < n),
                kernels_by_calls={r["Name"][:60]: int(r["Calls"]) / n for r in per})


def main():
    args = sys.argv[1:]
    with tempfile.TemporaryDirectory() as logdir:
        if args[0] in ("--trace", "--trace-target"):
            agent = make_agent(args[1], args[2], logdir)
            inds = agent.replay.draw(TRACE_WARM + TRACE_STEPS, agent.batch_size)
            call = target_only(agent, inds[0]) if args[0] == "--trace-target" else None
            for b in range(TRACE_WARM + TRACE_STEPS):
                call() if call else agent.update_minibatch(inds[b])
            torch.cuda.synchronize()
            return
        path = args[0]
        out = json.load(open(path)) if os.path.exists(path) else {}
        if len(args) > 1 and args[1] in ("--launches", "--launches-target"):
            c = count_launches(args[2], TRACE_WARM + TRACE_STEPS)
            what = "update" if args[1] == "--launches" else "actor_target"
            out.setdefault(f"{args[3]}/{args[4]}", {}).update({f"launches_per_{what}": c["launches"],
                                                              f"runtime_copy_launches_per_{what}": c["runtime_copy_launches"],
                                                              f"one_off_launches_{what}_trace": c["one_off_launches"],
                                                              f"kernels_by_calls_per_{what}": c["kernels_by_calls"]})
        else:
            out.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, measured_on=measured_on(),
                       method="median of 10 passes of >= 0.5 s between device events, every shape warmed")
            for shape in SHAPES:
                for prec in ("bf16", "fp32"):
                    agent = make_agent(shape, prec, logdir)
                    inds = agent.replay.draw(64, agent.batch_size)
                    it = iter(range(10 ** 9))
                    upd, reps_u = timed(lambda: agent.update_minibatch(inds[next(it) % 64]))
                    nxt = agent.replay.gather(inds[0])[1]
                    smp, _ = timed(lambda: agent.model(cond={"state": nxt}))
                    tgt, reps_t = timed(target_only(agent, inds[0]))
                    out.setdefault(f"{shape}/{prec}", {}).update(batch=agent.batch_size, ms_per_update=upd, updates_per_pass=reps_u,
                                                                 ms_per_sampler_call=smp, sampler_share_of_update=smp / upd,
                                                                 denoising_steps=agent.model.denoising_steps,
                                                                 ms_per_actor_target=tgt, actor_targets_per_pass=reps_t)
                    print(shape, prec, out[f"{shape}/{prec}"], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
