#!/usr/bin/env python3
"""Fingerprint of ``agent.run()`` for every fine-tuning agent whose host loop is shared code: a sha256 of every tensor of the final
``model.state_dict()`` and the run's records (without ``time``; the times are kept beside them).  Only the public path is used
(``load_config``, ``get_class(cfg._target_)(cfg).run()``), so the same file fingerprints any checkout: ``--root`` names the tree
whose ``dppo_amd`` and ``tests`` are imported (this one by default).  The cfgs are those of tests/test_agent_gpu.py (state diffusion
with 1 and 2 pipeline groups, Gaussian, GMM, conv denoiser, both pixel actors, pixel Gaussian, the two-rank pixel run) and the
shrunk shipped cfgs of tests/test_idql.py and tests/test_sac.py; seed 42; fp32 and bf16.

    python tools/agent_fingerprint.py --all out/here                       # every case, one process each, under its own timeout
    python tools/agent_fingerprint.py --all out/parent --root ../parent    # the same file against another checkout
    python tools/agent_fingerprint.py --compare out/parent out/here        # equal hashes / records per case, as JSON
"""
import argparse
import fnmatch
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PPO_CASES = ("ppo_groups1", "ppo_groups2", "gaussian", "gmm", "unet", "img_mlp", "img_unet_two_cameras", "img_gaussian")
CASES = PPO_CASES + ("idql", "sac", "img_mlp_2rank")
NETS = ("actor", "critic", "critic_q", "critic_v")  # the cfg.model nodes that take ``precision``
CASE_TIMEOUT = 240


def make_cfg(case, prec, tmp, rank=0):
    """The case's cfg, from the test module that defines it, with ``precision`` set on every network node."""
    os.environ["DPPO_LOG_DIR"] = tmp
    from dppo_amd.cfg.loader import load_config
    if case == "idql":
        from tests.test_idql import agent_cfg
        cfg = agent_cfg(tmp)
    elif case == "sac":
        from tests.test_sac import agent_cfg
        cfg = agent_cfg(tmp)
    else:
        from tests import test_agent_gpu as T
        img = lambda kind: T.IMG_YAML.replace("ACTOR", T.IMG_ACTORS[kind][0]).replace("NUM_IMG", str(T.IMG_ACTORS[kind][1])).replace(
            "RGB_C", str(3 * T.IMG_ACTORS[kind][1]))
        text = {
            "ppo_groups1": lambda: T.YAML.replace("  n_envs: 4\n", "  n_envs: 4\n  pipeline_groups: 1\n"),
            "ppo_groups2": lambda: T.YAML.replace("  n_envs: 4\n", "  n_envs: 4\n  pipeline_groups: 2\n"),
            "gaussian": lambda: T.GAUSS_YAML.replace("      vf_coef: 0.5\n", "      vf_coef: 0.5\n      ent_coef: 0.01\n"),
            "gmm": lambda: T.GMM_YAML,
            "unet": lambda: T.UNET_YAML.replace("n_steps: 12", "n_steps: 6"),
            "img_mlp": lambda: img("mlp"),
            "img_unet_two_cameras": lambda: img("unet_two_cameras"),
            "img_gaussian": lambda: T.GAUSS_IMG_YAML.replace("RGB_C", "3"),
            "img_mlp_2rank": lambda: img("mlp").replace("  n_train_itr: 3\n", "  n_train_itr: 2\n  force_train: True\n"),
        }[case]()
        path = os.path.join(tmp, f"cfg_{rank}.yaml")
        with open(path, "w") as f:
            f.write(text)
        cfg = load_config(path)
    for k in NETS:
        if k in cfg.model:
            cfg.model[k]["precision"] = prec
    return cfg


def run_case(case, prec, out, rank=None, port=None):
    import torch
    if rank is not None:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=2)  # (both ranks on the one device, as the test has it)
    from dppo_amd.cfg.loader import get_class
    with tempfile.TemporaryDirectory() as tmp:
        cfg = make_cfg(case, prec, tmp, rank or 0)
        agent = get_class(cfg._target_)(cfg)
        res = agent.run()
        torch.cuda.synchronize()
        tensors = dict(agent.model.state_dict())
        if hasattr(agent, "log_alpha"):
            tensors["agent.log_alpha"] = agent.log_alpha
        hashes = {k: hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
                  for k, t in tensors.items()}
    records = [{k: repr(v) for k, v in r.items() if k != "time"} for r in res]
    with open(out, "w") as f:
        json.dump({"case": case, "precision": prec, "rank": rank, "hashes": hashes, "records": records,
                   "time": [r.get("time") for r in res]}, f, indent=1)
    if rank is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_all(outdir, root, only):
    """One child process per run, each under its own timeout; the first failure ends the script."""
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    base = [sys.executable, os.path.abspath(__file__), "--root", root]
    for case in CASES:
        for prec in ("fp32", "bf16"):
            name = f"{case}.{prec}"
            if only and not any(fnmatch.fnmatch(name, o) for o in only):
                continue
            if case.endswith("_2rank"):
                s = socket.socket()
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
                s.close()
                cmds = [base + ["--case", case, "--prec", prec, "--rank", str(r), "--port", str(port), "--out",
                                os.path.join(outdir, f"{name}.rank{r}.json")] for r in range(2)]
            else:
                cmds = [base + ["--case", case, "--prec", prec, "--out", os.path.join(outdir, f"{name}.json")]]
            logs = [tempfile.TemporaryFile(mode="w+") for _ in cmds]  # files, not pipes: no rank can stall on a full pipe
            procs = [subprocess.Popen(c, stdout=f, stderr=subprocess.STDOUT) for c, f in zip(cmds, logs)]
            for p, f in zip(procs, logs):
                try:
                    p.wait(timeout=CASE_TIMEOUT)
                except subprocess.TimeoutExpired:
                    for q in procs:
                        q.kill()
                    sys.exit(f"{name}: no result within {CASE_TIMEOUT} s; stopping")
                if p.returncode != 0:
                    for q in procs:
                        q.kill()
                    f.seek(0)
                    sys.exit(f"{name}: exit status {p.returncode}; stopping\n{f.read()[-3000:]}")
            print(f"{name}: done", flush=True)


def steady_seconds(result):
    """The run's iterations behind the first timed one (whose first-use costs are left out): last ``time`` minus first."""
    t = [x for x in result["time"] if x is not None]
    return t[-1] - t[0] if len(t) > 1 else None


def compare(a_dir, b_dir):
    """Per result file of ``a_dir``: whether ``b_dir`` has the same hashes and the same records; where the records differ, the
    largest relative difference of a numeric field."""
    out = {}
    for name in sorted(os.listdir(a_dir)):
        if not name.endswith(".json") or not os.path.exists(os.path.join(b_dir, name)):
            continue
        a, b = (json.load(open(os.path.join(d, name))) for d in (a_dir, b_dir))
        worst = 0.0
        for ra, rb in zip(a["records"], b["records"]):
            for k in ra:
                if ra[k] != rb.get(k):
                    try:
                        x, y = float(ra[k]), float(rb.get(k, "nan"))
                    except ValueError:  # not a number: the records differ, and that is all there is to say
                        worst = float("inf")
                        continue
                    worst = max(worst, abs(x - y) / max(abs(x), abs(y), 1e-300))
        out[name[:-5]] = {"tensors": len(a["hashes"]), "hashes_equal": a["hashes"] == b["hashes"],
                          "records_equal": a["records"] == b["records"], "records_max_rel_diff": worst,
                          "steady_seconds": [steady_seconds(x) for x in (a, b)]}  # (None: a rank > 0 keeps no records)
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--all", metavar="OUTDIR")
    ap.add_argument("--only", nargs="*", default=[], metavar="PATTERN", help="with --all: run names (case.precision) to keep, as globs")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--prec", default="fp32")
    ap.add_argument("--rank", type=int)
    ap.add_argument("--port", type=int)
    ap.add_argument("--out")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.compare:
        compare(*args.compare)
    elif args.all:
        run_all(args.all, root, args.only)
    else:
        out = os.path.abspath(args.out)
        sys.path.insert(0, root)
        os.chdir(root)
        run_case(args.case, args.prec, out, args.rank, args.port)
