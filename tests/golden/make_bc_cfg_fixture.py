"""Regenerate tests/golden/shipped_bc_cfgs.json from a checkout of the reference's cfg/ tree:

    python tests/golden/make_bc_cfg_fixture.py <reference>/cfg

The Gaussian / mixture pre-training cfgs (pre_gaussian_mlp.yaml, pre_gmm_mlp.yaml) that tests/test_pretrain_gaussian.py walks,
by make_cfg_fixture.py's method: each one resolved by dppo_amd's own loader (device=cpu) and stored as plain values, keyed by
its path under cfg/ -- the keys that script keeps plus train.ent_coef where present.  shipped_cfgs.json holds neither pattern
and is not touched."""
import fnmatch
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dppo_amd.cfg.loader import load_config  # noqa: E402

PATTERNS = ("*/pretrain/*/pre_gaussian_mlp.yaml", "*/pretrain/*/pre_gmm_mlp.yaml")
TOP_KEYS = ("_target_", "denoising_steps", "horizon_steps", "action_dim", "num_modes", "model")


def main(src):
    os.environ.update(DPPO_LOG_DIR="/tmp/log", DPPO_DATA_DIR="/tmp/data", DPPO_WANDB_ENTITY="none")
    out = {}
    for path in sorted(glob.glob(os.path.join(src, "*", "*", "*", "*.yaml"))):
        rel = os.path.relpath(path, src)
        if not any(fnmatch.fnmatch(rel, p) for p in PATTERNS):
            continue
        cfg = load_config(path, overrides=["device=cpu"])
        keep = {k: cfg[k] for k in TOP_KEYS if k in cfg}
        train = {k: cfg.train[k] for k in ("batch_size", "ent_coef") if k in cfg.get("train", {})}
        if train:
            keep["train"] = train
        if "ema" in cfg:
            keep["ema"] = {"decay": cfg.ema.decay}
        out[rel] = keep
    with open(os.path.join(ROOT, "tests", "golden", "shipped_bc_cfgs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cfgs")


if __name__ == "__main__":
    main(sys.argv[1])
