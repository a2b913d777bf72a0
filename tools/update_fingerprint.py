#!/usr/bin/env python3
"""Bit-level fingerprint of the training entry points: one update per case on fixed seeds, a sha256 of every output tensor
(statistics, each actor gradient, each critic gradient) and the workspace size.  Two builds of the library compute the same
thing exactly when their fingerprints are equal; DPPO_HIP_LIB selects the build, one build per process.

    python tools/update_fingerprint.py --out a.json [--only hopper/bf16,rlpd_] [--knobs default,38=0,1=0]
    python tools/update_fingerprint.py --compare a.json b.json

Cases: ppo_update in rollout mode for seven network pairs in both precisions under eleven knob sets (hopper and halfcheetah at
N = 1300 -- 21 row tiles, the last of 20 rows; the others at N = 6500, enough for the low-rank route at their width), and at the
default knobs one case per other entry point, each built from its own test module's helpers; for the LayerNorm-critic family
(RLPD's, Cal-QL's and IBRL's critic and actor / acting entries) and the plain twin-Q family (QSM's, DQL's and SAC's) the two smallest
fixture cases of each, with the workspace size."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dppo_amd import hip  # noqa: E402
from tests.conftest import load_golden  # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"
KNOB_SETS = ["default", "1=0", "2=0", "11=0", "12=0", "14=0", "16=0", "18=0", "37=0", "38=0", "41=0"]
PPO_SPECS = {"hopper": 1300, "halfcheetah": 1300, "can": 6500, "can_relu": 6500, "kitchen_like": 6500, "square_like": 6500,
             "transport": 6500, "ln_relu": 1300}  # ln_relu (LayerNorm blocks): default knobs only


def sha(t):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t, dtype=np.float64))
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def wanted(only, name):
    """``only``: substrings of case names, comma-separated; the empty string takes every case"""
    return any(o in name for o in only.split(","))


def grads_of(tag, net, out, flat=None):
    """one hash per parameter tensor: of its .grad, or of its slice of a flat gradient"""
    off = 0
    for k, p in net.named_parameters():
        if flat is not None:
            if off + p.numel() > flat.numel():
                break  # (parameters outside the trunk, such as logvar)
            out[f"{tag}.{k}"] = sha(flat[off:off + p.numel()])
            off += p.numel()
        elif p.grad is not None:
            out[f"{tag}.{k}"] = sha(p.grad)


def ppo_cases(only, knob_sets):
    from tests.test_hip_parity import build_model
    lib = hip.load()
    for sname, N in PPO_SPECS.items():
        for prec in ("fp32", "bf16"):
            sets = [k for k in knob_sets if sname != "ln_relu" or k == "default"]
            names = {k: f"ppo/{sname}/{prec}/{k}" for k in sets}
            if not any(wanted(only, n) for n in names.values()):
                continue
            Kft, R = 10, 800
            m, a, c = build_model(sname, dict(denoising_steps=20, ft_denoising_steps=Kft, randn_clip_value=3), 73, prec)
            AF = a.horizon_steps * a.action_dim
            gen = torch.Generator(device="cpu").manual_seed(5)
            obs = (torch.rand(R, 1, a.cond_dim, generator=gen) * 2 - 1).to(DEV)
            chains = (torch.randn(R, Kft + 1, a.horizon_steps, a.action_dim, generator=gen) * 0.5).to(DEV)
            logp = m.get_logprobs({"state": obs}, chains).reshape(R, Kft, AF) + 0.01
            val = m.critic({"state": obs}).reshape(R)
            ret = val + torch.randn(R, generator=gen).to(DEV)
            adv = torch.randn(R, generator=gen).to(DEV)
            inds = torch.randperm(R * Kft, generator=gen)[:N].to(DEV).contiguous()
            ws = lib.dppo_ppo_workspace_bytes(C.byref(m.actor_ft.net_desc()), C.byref(m.critic.net_desc()), hip.PREC_BY_NAME[prec], N)
            for k in sets:
                if not wanted(only, names[k]):
                    continue
                knob = [int(x) for x in k.split("=")] if k != "default" else None
                try:
                    if knob:
                        assert lib.dppo_tune_set(*knob) == 0
                    for net in (m.actor, m.actor_ft, m.critic):
                        net.mark_updated()  # (the packed image depends on knob 1)
                    st = m.ppo_update(obs.reshape(R, -1).contiguous(), chains.reshape(R, Kft + 1, AF).contiguous(), ret, val, adv,
                                      logp, inds)
                    out = {"stats": sha(st), "workspace_bytes": ws}
                    grads_of("actor", m.actor_ft, out, m.actor_ft.flat_grads())
                    grads_of("critic", m.critic, out, m.critic.flat_grads())
                finally:
                    if knob:
                        lib.dppo_tune_set(knob[0], 1)
                yield names[k], out


def bc_case(prec):
    from tests.test_hip_parity import build_model
    from tests.test_oracle_golden import BC_CASES
    g = load_golden("g8_bc")
    sname, kw = BC_CASES["bc_ddpm"]
    m, a, _ = build_model(sname, dict(kw, clip_ploss_coef=0.01), 41, prec)
    value, grad = m.bc_loss_and_grad({"state": T(g["bc_ddpm_state"]).to(DEV)}, noise=T(g["bc_ddpm_noise"]).to(DEV))
    out = {"loss": sha(value)}
    grads_of("actor", m.actor_ft, out, grad)
    return out


def mse_case(case, prec):
    from tests.test_hip_parity import build_model
    from tests.test_oracle_golden import MSE_CASES
    g = load_golden("g9_denoise_mse")
    sname, K = MSE_CASES[case]
    d = lambda k: T(g[f"{case}_{k}"]).to(DEV)
    m, a, _ = build_model(sname, dict(denoising_steps=K, ft_denoising_steps=min(10, K)), 51, prec)
    for p in m.network.parameters():
        p.requires_grad_(True)
    loss = m.p_losses(d("x0"), {"state": d("state")}, d("t"), noise=d("noise"))
    loss.backward()
    out = {"loss": sha(loss)}
    grads_of("net", m.network, out)
    return out


def vision_mse_case(prec):  # the denoising loss WITH d_obs: a visual encoder back-propagates from it
    from tests.golden.make_golden_cases import VIS_MSE_CASES
    from tests.test_vision import cuda_cond, hip_vision_model
    g, case = load_golden("g17_vision_loss"), "vmlp_mse"
    name, K, N = VIS_MSE_CASES[case]
    m, *_ = hip_vision_model(name, 51, prec, dict(denoising_steps=K, ft_denoising_steps=min(10, K), clip_ploss_coef=0.01))
    for p in m.network.parameters():
        p.requires_grad_(True)
    d = lambda k: T(g[f"{case}_{k}"]).cuda()
    loss = m.p_losses(d("x0"), cuda_cond(g, case, u8=True), d("t"), noise=d("noise"))
    loss.backward()
    out = {"loss": sha(loss)}
    grads_of("net", m.network, out)
    return out


def vision_ppo_case(prec):  # the gathered-mode _obs entry with d_obs_actor and d_obs_critic
    from tests.golden.make_golden_cases import VIS_LOSS_CASES
    from tests.test_vision import cuda_cond, hip_vision_model
    g, case = load_golden("g17_vision_loss"), "vmlp_loss"
    name, N, kw, rh = VIS_LOSS_CASES[case]
    m, *_ = hip_vision_model(name, 31, prec, kw)
    d = lambda k: T(g[f"{case}_{k}"]).cuda()
    res = m.loss(cuda_cond(g, case, u8=True), d("prev"), d("next"), d("kinds"), d("returns"), d("oldvalues"), d("adv"),
                 d("oldlogprobs"), use_bc_loss=False, reward_horizon=rh)
    (res[0] + 0.5 * res[2]).backward()
    out = {"stats": sha([float(x) for x in res[:8]])}
    grads_of("actor", m.actor_ft, out)
    grads_of("critic", m.critic, out)
    return out


def gaussian_case(case, prec):
    from tests.test_gaussian import build
    g = load_golden("g12_gaussian")
    m, a, c = build(case, prec)
    d = lambda k: T(g[f"{case}_{k}"]).to(DEV)
    res = m.loss({"state": d("state")}, d("actions"), d("returns"), d("oldvalues"), d("adv"), d("oldlogprobs"))
    (res[0] + 0.01 * res[1] + 0.5 * res[2]).backward()
    out = {"stats": sha([float(x) for x in res[:8]])}
    grads_of("actor", m.actor_ft, out)
    grads_of("critic", m.critic, out)
    return out


def gmm_case(case, prec):
    from tests.test_gmm import build
    g = load_golden("g20_gmm")
    m = build(case, prec)
    d = lambda k: T(g[f"{case}_{k}"]).cuda()
    m.ent_coef = 0.01
    res = m.loss({"state": d("state")}, d("actions"), d("returns"), d("oldvalues"), d("adv"), d("oldlogprobs"))
    (res[0] + 0.5 * res[2]).backward()
    out = {"stats": sha([float(x) for x in res[:8]])}
    grads_of("actor", m.actor_ft, out)
    grads_of("critic", m.critic, out)
    return out


def idql_case(net, n, prec):
    from tests import test_idql as I
    g = load_golden("g24_idql")
    m = I.build_model(net, prec, float(g[f"{net}_{n}_v_bias"]))
    res = I.run_losses(m, I.case_batch(g, net, n))
    out = {k: sha(res[k]) for k in ("adv", "v_loss", "v_stats", "q_loss", "q_stats")}
    for tag, mod, flat in (("v", m.critic_v, res["gv"]), ("q", m.critic_q, res["gq"])):
        for k, gv in I.named_grads(mod, flat):
            out[f"{tag}.{k}"] = sha(gv)
    return out


def plain_case(case, prec):
    from tests.test_plain_mlp import build
    g = load_golden("g19_plain_mlp")
    m, a, c = build(case, prec)
    d = lambda k: T(g[f"{case}_{k}"]).cuda()
    res = m.loss({"state": d("state")}, d("prev"), d("next"), d("kinds"), d("returns"), d("oldvalues"), d("adv"), d("oldlogprobs"),
                 use_bc_loss=False, reward_horizon=4)
    (res[0] + 0.5 * res[2]).backward()
    out = {"stats": sha([float(x) for x in res[:8]])}
    grads_of("actor", m.actor_ft, out)
    grads_of("critic", m.critic, out)
    return out


# The LayerNorm-critic family (RLPD, Cal-QL, IBRL): one fresh model per case, so that its grow-only workspace has the size the
# entry's query answered; every tensor the entry writes.
def rlpd_q_case(case, n, prec):
    from tests import test_rlpd as R
    m = R.make_model(case, prec, DEV, R.K.backup_entropy(case, n))
    res = R.run_critic(m, case, n)
    out = {"loss": sha(res["loss"]), "stats": sha(res["stats"]), "workspace_bytes": m._ws_q.buf.numel()}
    out.update((f"q.{k}", sha(g)) for k, g in R.named_grads(m))
    return out


def rlpd_actor_case(case, n, prec):
    from tests import test_rlpd_actor as R
    m = R.make_model(case, prec, DEV)
    res = R.run_actor(m, R.dev_inputs(case, n))
    out = {k: sha(v) for k, v in res.items()}
    out["workspace_bytes"] = m._ws_actor.buf.numel()
    return out


def calql_q_case(case, n, prec):
    from tests import test_calql as Q
    m = Q.make_model(case, n, prec, DEV)
    res = Q.run_critic(m, case, n, False)
    out = {"loss": sha(res["loss"]), "stats": sha(res["stats"]), "y": sha(res["y"]), "workspace_bytes": m._ws_calql.buf.numel()}
    out.update((f"q.{k}", sha(g)) for k, g in Q.named_grads(m))
    return out


def calql_actor_case(case, prec):
    from tests import test_calql_actor as Q
    m = Q.make_model(case, prec, DEV)
    res = Q.run_actor(m, Q.dev_inputs(case))
    out = {k: sha(v) for k, v in res.items()}
    out["workspace_bytes"] = m._ws_actor.buf.numel()
    return out


def ibrl_act_case(case, n, soft, prec):
    from tests import test_ibrl as B
    m = B.make_model(case, prec, DEV, soft)
    out = {k: sha(v) for k, v in B.run_forward(m, case, n).items()}
    out["workspace_bytes"] = m._ws_act.buf.numel()
    return out


def ibrl_q_case(case, n, prec):
    from tests import test_ibrl as B
    m = B.make_model(case, prec, DEV)
    res = B.run_critic(m, case, n)
    out = {"loss": sha(res["loss"]), "stats": sha(res["stats"]), "y": sha(res["y"]), "bc_share": sha(res["share"]),
           "workspace_bytes": m._ws_q.buf.numel()}
    out.update((f"q.{k}", sha(g)) for k, g in B.named_grads(m))
    return out


def ibrl_actor_case(case, n, prec):
    from tests import test_ibrl_actor as B
    m = B.make_model(case, prec, DEV)
    res = B.run_actor(m, B.dev_inputs(case, n))
    out = {k: sha(v) for k, v in res.items() if v is not None}
    out["workspace_bytes"] = m._ws_actor.buf.numel()
    return out


def ln_family_cases(table, prec):
    for case, n in (("tiny", 77), ("chunk", 77)):  # chunk_77: RLPD's case without the entropy backup
        table[f"rlpd_q/{case}_{n}/{prec}"] = lambda c=case, k=n: rlpd_q_case(c, k, prec)
        table[f"rlpd_actor/{case}_{n}/{prec}"] = lambda c=case, k=n: rlpd_actor_case(c, k, prec)
        table[f"calql_q/{case}_{n}/{prec}"] = lambda c=case, k=n: calql_q_case(c, k, prec)
        table[f"calql_actor/{case}_{n}/{prec}"] = lambda c=case, k=n: calql_actor_case(f"{c}_{k}", prec)
    for case, n in (("tiny", 77), ("chunk", 130)):  # E = 3 and 5: the stream rotation wraps; N off a tile boundary
        for soft in (False, True):
            table[f"ibrl_act/{case}_{n}_{'soft' if soft else 'greedy'}/{prec}"] = lambda c=case, k=n, s=soft: ibrl_act_case(c, k, s, prec)
        table[f"ibrl_q/{case}_{n}/{prec}"] = lambda c=case, k=n: ibrl_q_case(c, k, prec)
        table[f"ibrl_actor/{case}_{n}/{prec}"] = lambda c=case, k=n: ibrl_actor_case(c, k, prec)


# The plain twin-Q family (QSM, DQL, SAC): as above, one fresh model per case and every tensor the entry writes.
def hashed(res, ws):
    out = {k: sha(v) for k, v in res.items()}
    out["workspace_bytes"] = ws.buf.numel()
    return out


def qsm_case(which, net, n, prec):
    from tests import test_qsm as Q
    m, b = Q.make_model(net, prec, DEV), Q.dev_batch(net, n)
    if which == "q":
        return hashed(Q.run_critic(m, b), m._ws_q)
    return hashed(Q.run_actor(m, net, b), m._ws_target)


def dql_case(case, n, prec):
    from tests import test_dql as D
    m = D.make_model(case, prec, DEV)
    return hashed(D.run_actor(m, case, n, D.given_chain(load_golden("g26_dql"), case, n)), m._ws_actor)


def sac_case(which, case, n, prec):
    from tests import test_sac as S
    m, b = S.make_model(case, prec, DEV), S.dev_batch(case, n)
    if which == "sample":
        return hashed(dict(zip(("a", "logp", "u"), S.run_sample(m, b))), m._ws_s)
    if which == "q":
        return hashed(S.run_critic(m, b), m._ws_q)
    return hashed(S.run_actor(m, b), m._ws_actor)


def twin_q_cases(table, prec):
    for net in ("scratch", "transport"):  # transport: Q in_dim 171, wider than one k tile
        for which in ("q", "actor"):
            table[f"qsm_{which}/{net}_77/{prec}"] = lambda w=which, c=net: qsm_case(w, c, 77, prec)
    for case in ("scratch", "hopper"):
        table[f"dql_actor/{case}_77/{prec}"] = lambda c=case: dql_case(c, 77, prec)
    for case in ("tiny", "chunk"):
        for which in ("sample", "q", "actor"):
            table[f"sac_{which}/{case}_77/{prec}"] = lambda w=which, c=case: sac_case(w, c, 77, prec)


def other_cases(only):
    from tests.golden import make_golden_idql_cases as K
    table = {}
    for prec in ("fp32", "bf16"):
        table[f"bc/hopper/{prec}"] = lambda p=prec: bc_case(p)
        for case in ("mse_hopper", "mse_can_k100", "mse_ln_relu"):
            table[f"mse/{case}/{prec}"] = lambda c=case, p=prec: mse_case(c, p)
        table[f"mse_dobs/vmlp_mse/{prec}"] = lambda p=prec: vision_mse_case(p)
        table[f"ppo_obs/vmlp_loss/{prec}"] = lambda p=prec: vision_ppo_case(p)
        for case in ("gauss_d3il_fixed", "gauss_furniture_learned"):
            table[f"gaussian/{case}/{prec}"] = lambda c=case, p=prec: gaussian_case(c, p)
        for case in ("gmm_can", "gmm_d3il"):
            table[f"gmm/{case}/{prec}"] = lambda c=case, p=prec: gmm_case(c, p)
        net, n = K.IDQL_CASES[-1]
        table[f"idql/{net}_{n}/{prec}"] = lambda a=net, b=n, p=prec: idql_case(a, b, p)
        for case in ("plain_ddpm", "plain_small_ddim"):
            table[f"plain/{case}/{prec}"] = lambda c=case, p=prec: plain_case(c, p)
        ln_family_cases(table, prec)
        twin_q_cases(table, prec)
    for name, fn in table.items():
        if wanted(only, name):
            yield name, fn()


def compare(a, b):
    fa, fb = json.load(open(a)), json.load(open(b))
    bad = [f"{case}: {key}" for case in sorted(set(fa) | set(fb))
           for key in sorted(set(fa.get(case, {})) | set(fb.get(case, {}))) if fa.get(case, {}).get(key) != fb.get(case, {}).get(key)]
    print(f"{len(fa)} / {len(fb)} cases, {len(bad)} differing entries" + "".join("\n  " + x for x in bad[:200]))
    return 1 if bad or not fa else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="", help="substrings of the case names to run, comma-separated")
    ap.add_argument("--knobs", default=",".join(KNOB_SETS))
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    fp = {}
    for gen in (ppo_cases(args.only, args.knobs.split(",")), other_cases(args.only)):
        for name, out in gen:
            fp[name] = out
            print(name, len(out), flush=True)
    torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(fp, open(args.out, "w"), indent=0, sort_keys=True)
    print(f"{len(fp)} cases from {hip.LIB_PATH}")


if __name__ == "__main__":
    main()
