"""Regenerate tests/golden/shipped_ibrl_cfgs.json from a checkout of the reference's cfg/ tree:

    python tests/golden/make_ibrl_cfg_fixture.py <reference>/cfg

All eight IBRL cfgs the reference ships (*/ibrl_mlp*.yaml), which tests/test_ibrl.py walks, by make_idql_cfg_fixture.py's method and
keys: resolved by dppo_amd's own loader (device=cpu) and stored as plain values, keyed by its path under cfg/ -- settings only:
the agent target, the shapes, the whole train section and the model node."""
import fnmatch
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dppo_amd.cfg.loader import load_config  # noqa: E402

PATTERNS = ("*/*/*/ibrl_mlp*.yaml",)
TOP_KEYS = ("_target_", "obs_dim", "action_dim", "cond_steps", "horizon_steps", "act_steps", "train", "model")


def main(src):
    os.environ.update(DPPO_LOG_DIR="/tmp/log", DPPO_DATA_DIR="/tmp/data", DPPO_WANDB_ENTITY="none")
    out = {}
    for path in sorted(glob.glob(os.path.join(src, "*", "*", "*", "*.yaml"))):
        rel = os.path.relpath(path, src)
        if not any(fnmatch.fnmatch(rel, p) for p in PATTERNS):
            continue
        cfg = load_config(path, overrides=["device=cpu"])
        keep = {k: cfg[k] for k in TOP_KEYS if k in cfg}
        keep["env"] = {"n_envs": cfg.env.n_envs}
        out[rel] = keep
    with open(os.path.join(ROOT, "tests", "golden", "shipped_ibrl_cfgs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cfgs")


if __name__ == "__main__":
    main(sys.argv[1])
