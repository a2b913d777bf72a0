"""Regenerate tests/golden/shipped_cfgs.json from a checkout of the reference's cfg/ tree:

    python tests/golden/make_cfg_fixture.py <reference>/cfg

Every cfg tests/test_cfg_loader.py walks is resolved by dppo_amd's own loader (with the overrides that test applies) and
stored as plain values, keyed by its path under cfg/: the keys the tests read and nothing else, no interpolations left."""
import fnmatch
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dppo_amd.cfg.loader import load_config  # noqa: E402

PATTERNS = {  # pattern -> overrides the test loads it with
    "*/finetune/*/ft_ppo_diffusion_mlp.yaml": [],
    **{p: ["device=cpu"] for p in (
        "*/pretrain/*/pre_diffusion_mlp.yaml", "*/finetune/*/ft_ppo_diffusion_unet.yaml", "*/pretrain/*/pre_diffusion_unet.yaml",
        "*/finetune/*/ft_ppo_gaussian_mlp.yaml", "*/eval/*/eval_diffusion_mlp.yaml", "*/eval/*/eval_diffusion_unet.yaml",
        "*/finetune/*/ft_ppo_diffusion_mlp_img.yaml", "*/finetune/*/ft_ppo_diffusion_unet_img.yaml",
        "*/pretrain/*/pre_diffusion_mlp_img.yaml", "*/pretrain/*/pre_diffusion_unet_img.yaml",
        "*/eval/*/eval_diffusion_mlp_img.yaml", "*/eval/*/eval_diffusion_unet_img.yaml",
        "*/finetune/*/ft_ppo_gaussian_mlp_img.yaml", "*/finetune/*/ft_ppo_gmm_mlp.yaml")},
}
TOP_KEYS = ("_target_", "denoising_steps", "horizon_steps", "action_dim", "num_modes", "model")


def main(src):
    os.environ.update(DPPO_LOG_DIR="/tmp/log", DPPO_DATA_DIR="/tmp/data", DPPO_WANDB_ENTITY="none")
    out = {}
    for path in sorted(glob.glob(os.path.join(src, "*", "*", "*", "*.yaml"))):
        rel = os.path.relpath(path, src)
        pats = [p for p in PATTERNS if fnmatch.fnmatch(rel, p)]
        if not pats:
            continue
        cfg = load_config(path, overrides=PATTERNS[pats[0]])
        keep = {k: cfg[k] for k in TOP_KEYS if k in cfg}
        if "batch_size" in cfg.get("train", {}):
            keep["train"] = {"batch_size": cfg.train.batch_size}
        if "ema" in cfg:
            keep["ema"] = {"decay": cfg.ema.decay}
        out[rel] = keep
    with open(os.path.join(ROOT, "tests", "golden", "shipped_cfgs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cfgs")


if __name__ == "__main__":
    main(sys.argv[1])
