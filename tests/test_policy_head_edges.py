"""The Gaussian and mixture-of-Gaussians policy heads (csrc/gaussian.hip, csrc/gmm.hip: sample, logprob, PPO loss, BC loss)
against ``oracle/dppo_oracle.py`` run in FLOAT64 on the CPU, at the shapes the recorded fixtures never reach: ragged N (the
Gaussian kernels pack 16 samples per block, the mixture kernels 4), Ta*Da on both sides of the 16-lane stride, M*Ta*Da on both
sides of the 64-lane stride, M = 1 and M = 8, ``tanh_output=False``, and a learned std whose ``logvar`` entries fall below,
inside and above the clamp.

The inputs are BUILT, not drawn: the float64 means come first, then ``actions = mean_k + sigma * s * u`` with the per-sample
scale ``s`` solved so that log p lands where the case wants it (inside the [-5, 2] window, above it, below it, hundreds of nats
below it), ``oldlogp = clamp(logp) + off`` with ``off`` cycling through +-0.05 (inside clip 0.1) and +-0.3 (outside), a few
``oldlogp`` beyond the window, advantages of both signs, ``oldvalues = v +- {0.1, 0.5}`` against a value clip of 0.2 and
``returns = v + {0.3, -0.3, 1.0}``.  ``test_cases_populate_every_regime_and_no_sample_is_fragile`` (CPU) asserts on the float64
oracle alone that every regime is populated in its designated case and that every sample sits at least a guard band -- ten times
the fp32 tolerance of the quantity that decides -- away from every decision the kernels take in float32.  No sample is ever left
out of a comparison.

Everything the reference sees is the float32 value the kernels see, cast to float64.  fp32 tolerances are the fixture tests'
(tests/test_gaussian.py, tests/test_gmm.py); they are ceilings, not measurements.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import dppo_oracle as O

F64 = torch.float64
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
CLIP, CV = 0.1, 0.2  # clip_ploss_coef of every case; clip_vloss_coef where a case has one
OFF = (0.05, -0.05, 0.3, -0.3)  # oldlogp = clamp(logp) + OFF[i % 4]: ratio = exp(-off), inside / outside [0.9, 1.1]
ADV = (1.0, -0.8, 0.5, -1.4, 0.3, -0.45, 1.2)  # period 7 against OFF's 4: every (off, sign) pair within 28 samples
OLDV = (0.1, -0.1, 0.5, -0.5)  # oldvalues = v + OLDV[i % 4]: |v - oldv| inside / outside CV
RET = (0.3, -0.3, 1.0)  # returns = v + RET[i % 3]: with the clip active, lu > lc and lu < lc both occur
ENT_COEF = 0.01  # of the PPO loss (as the fixture tests); the Gaussian BC loss takes BC_ENT_COEF
BC_ENT_COEF = 0.05

# fp32 ceilings: the bounds tests/test_gaussian.py and tests/test_gmm.py hold the same quantity of the same head to
TOL = {
    "gaussian": dict(act=2e-5, lp=2e-4, stat=(2e-4, 2e-5)),
    "gmm": dict(act=2e-4, lp=2e-3, stat=(2e-3, 2e-4)),
}
# guard bands: ten times the tolerance of the deciding quantity.  log p / oldlogp against the window edges: the log-prob
# tolerance.  ratio = exp(logratio) inherits the log-prob's absolute error times ratio.  v - oldv against +-cv and lu against
# lc: v is held to the statistics' tolerance.  logvar is a float32 input the kernel reads exactly; only the clamp bounds differ
# between float32 and float64, by one ulp of |log sigma^2| < 8 (1e-6): its band is 1e-3.
BAND_LP = {f: 10 * TOL[f]["lp"] for f in TOL}
BAND_V = {f: 10 * TOL[f]["stat"][0] for f in TOL}
BAND_LOGVAR = 1e-3
BAND_ADV = 1e-2  # |normalised advantage|: its sign picks the surrogate's branch; mean and std are float64 sums of 33 numbers

TRUNK = [128, 128, 128]  # the smallest residual trunk check_net() accepts; the mixture's plain trunk is [64, 64]


# ------------------------------------------------------------------------------------------------------------------ cases
def _g(N, Ni, Ta, Da, cond, act, tanh, learn, std, vclip, norm, lp):
    return dict(N=N, Ni=Ni, Ta=Ta, Da=Da, cond=cond, act=act, tanh=tanh, learn=learn, std=std, vclip=vclip, norm=norm, lp=lp)


# N: samples of the PPO loss; Ni: samples of sample / logprob / BC loss (the first rows of the same batch).  lp: the cycle of
# log-prob targets ("in", "above", "below", "far" = hundreds of nats below).  "above" needs a small sigma: log p is a MEAN over
# the elements, at most -log sigma - 0.92.
GAUSS = {
    "n2_1x1_learn": _g(2, 1, 1, 1, 3, "Mish", True, True, 0.1, CV, True, ("in", "in")),
    "n15_3x5_learn_notanh": _g(15, 17, 3, 5, 4, "ReLU", False, True, 0.1, None, False, ("in", "below", "in", "far", "in")),
    "n16_4x4_fixed": _g(16, 1, 4, 4, 5, "Mish", True, False, 0.04, CV, True, ("in", "above", "below", "in", "above")),
    "n17_1x17_learn_notanh": _g(17, 17, 1, 17, 3, "Mish", False, True, 0.1, CV, True, ("in", "in", "below", "in", "far")),
    "n33_2x20_learn": _g(33, 17, 2, 20, 5, "ReLU", True, True, 0.04, CV, True, ("in", "above", "in", "below", "in", "far")),
    "n33_3x5_fixed_notanh": _g(33, 1, 3, 5, 4, "Mish", False, False, 0.04, None, False, ("in", "above", "below", "in", "in")),
    "n17_4x4_learn": _g(17, 17, 4, 4, 3, "Mish", True, True, 0.04, None, False, ("above", "in", "below", "in")),
    "n15_1x1_fixed_notanh": _g(15, 17, 1, 1, 4, "ReLU", False, False, 0.04, CV, True, ("in", "above", "in", "below")),
    "n2_2x20_fixed": _g(2, 1, 2, 20, 3, "Mish", True, False, 0.1, None, True, ("in", "below")),
    "n16_1x17_learn": _g(16, 17, 1, 17, 5, "ReLU", True, True, 0.04, CV, False, ("in", "above", "below", "in", "far")),
    "n33_1x1_learn_notanh": _g(33, 17, 1, 1, 5, "Mish", False, True, 0.04, CV, True, ("in", "below", "in", "above", "in")),
}


def _m(N, Ni, M, Ta, Da, cond, res, learn, std, vclip, norm, lp, bias=None, far=False):
    return dict(N=N, Ni=Ni, M=M, Ta=Ta, Da=Da, cond=cond, res=res, act="Mish" if res else "ReLU", learn=learn, std=std, vclip=vclip,
                norm=norm, lp=lp, bias=bias, far=far)


# M * Ta * Da = 1, 64, 65, 16, 168: one lane, exactly one pass of the wave, one element into the second pass, ...
# bias: added to the weights trunk's output bias (mixture logits of -30 and -100: pi_m underflows).  far: every action at +-2,
# at distance >= 1 from every tanh mean with sigma 0.1 -- every component log-density hundreds of nats below zero.
GMM = {
    "n2_m1_1x1_learn": _m(2, 1, 1, 1, 1, 3, False, True, 0.04, CV, True, ("in", "above")),
    "n3_m8_1x8_learn": _m(3, 5, 8, 1, 8, 4, False, True, 0.1, None, True, ("in", "below", "above", "in", "in")),
    "n4_m5_1x13_fixed": _m(4, 1, 5, 1, 13, 5, False, False, 0.1, CV, False, ("above", "in", "below", "in")),
    "n5_m2_4x2_learn": _m(5, 5, 2, 4, 2, 3, False, True, 0.1, CV, True, ("in", "in", "below", "above", "in")),
    "n9_m8_3x7_learn": _m(9, 5, 8, 3, 7, 4, False, True, 0.1, CV, True, ("in", "in", "above", "in", "below", "in", "in", "in", "in")),
    "n9_m5_1x13_learn_res": _m(9, 5, 5, 1, 13, 5, True, True, 0.1, None, True, ("in", "below", "in", "above", "in")),
    "n9_m2_4x2_fixed": _m(9, 1, 2, 4, 2, 4, False, False, 0.1, CV, True, ("in", "in", "in", "in", "above", "below", "in", "far", "in")),
    "n9_m1_1x1_fixed": _m(9, 5, 1, 1, 1, 5, False, False, 0.04, CV, False, ("in", "above", "in", "below", "in", "far")),
    "n9_m5_1x13_fixed_bias": _m(9, 5, 5, 1, 13, 3, False, False, 0.1, CV, True, ("in", "in", "above", "in", "below"),
                                bias=(0.0, -30.0, -100.0, 0.5, -30.0)),
    "n5_m8_1x8_fixed_far": _m(5, 5, 8, 1, 8, 4, False, False, 0.1, None, True, (), far=True),
    "n3_m2_4x2_fixed_res": _m(3, 1, 2, 4, 2, 3, True, False, 0.1, None, False, ("in", "far", "in")),
    "n4_m8_3x7_fixed": _m(4, 5, 8, 3, 7, 5, False, False, 0.1, None, True, ("in", "above", "below", "in", "far")),
}
CASES = {"gaussian": GAUSS, "gmm": GMM}
ALL = [(f, n) for f in ("gaussian", "gmm") for n in CASES[f]]
ids = lambda fc: f"{fc[0]}-{fc[1]}"
RAGGED_LEARNED = [(f, n) for f, n in ALL if CASES[f][n]["learn"] and CASES[f][n]["N"] % (16 if f == "gaussian" else 4)]

# where each regime is asserted (the CPU test): {family: {regime: case}}
HOME = {
    "gaussian": {
        "logp_in": "n33_2x20_learn", "logp_above": "n33_2x20_learn", "logp_below": "n33_2x20_learn", "logp_far": "n33_2x20_learn",
        "old_above": "n33_2x20_learn", "old_below": "n33_2x20_learn",
        "ratio_lo_adv+": "n33_2x20_learn", "ratio_lo_adv-": "n33_2x20_learn", "ratio_in_adv+": "n33_2x20_learn",
        "ratio_in_adv-": "n33_2x20_learn", "ratio_hi_adv+": "n33_2x20_learn", "ratio_hi_adv-": "n33_2x20_learn",
        "vclip_inactive": "n33_2x20_learn", "vclip_active_lu>lc": "n33_2x20_learn", "vclip_active_lu<lc": "n33_2x20_learn",
        "logvar_below": "n17_1x17_learn_notanh", "logvar_inside": "n17_1x17_learn_notanh", "logvar_above": "n17_1x17_learn_notanh",
    },
    "gmm": {
        "logp_in": "n9_m2_4x2_fixed", "logp_above": "n9_m2_4x2_fixed", "logp_below": "n9_m2_4x2_fixed", "logp_far": "n9_m2_4x2_fixed",
        "old_above": "n9_m8_3x7_learn", "old_below": "n9_m8_3x7_learn",
        "ratio_lo_adv+": "n9_m8_3x7_learn", "ratio_lo_adv-": "n9_m5_1x13_learn_res", "ratio_in_adv+": "n9_m8_3x7_learn",
        "ratio_in_adv-": "n9_m8_3x7_learn", "ratio_hi_adv+": "n9_m5_1x13_learn_res", "ratio_hi_adv-": "n9_m8_3x7_learn",
        "vclip_inactive": "n9_m8_3x7_learn", "vclip_active_lu>lc": "n9_m8_3x7_learn", "vclip_active_lu<lc": "n9_m8_3x7_learn",
        "logvar_below": "n9_m8_3x7_learn", "logvar_inside": "n9_m8_3x7_learn", "logvar_above": "n9_m8_3x7_learn",
    },
}


# ------------------------------------------------------------------------------------------------- specs, weights, inputs
def specs(family, name):
    k = CASES[family][name]
    crit = O.NetSpec("critic", cond_dim=k["cond"], mlp_dims=list(TRUNK), activation="Mish", residual=True)
    if family == "gaussian":
        a = O.NetSpec("gaussian", cond_dim=k["cond"], mlp_dims=list(TRUNK), activation=k["act"], residual=True, action_dim=k["Da"],
                      horizon_steps=k["Ta"])
        return a, crit
    dims = list(TRUNK) if k["res"] else [64, 64]
    ms, ws = O.gmm_specs(k["cond"], dims, k["act"], k["res"], k["Da"], k["Ta"], k["M"])
    return (ms, ws), crit


def std_range(k):
    return 0.67 * k["std"], 1.33 * k["std"]


def weights(family, name):
    """(actor state dict, critic state dict, logvar or None), float32: what the model loads and -- cast to float64 -- the oracle."""
    k = CASES[family][name]
    a, crit = specs(family, name)
    if family == "gaussian":
        sd, n_lv = dict(O.init_params(a, 71)), k["Da"]
    else:
        sd, n_lv = dict(O.gmm_init_params(a[0], a[1], 71)), k["M"] * k["Da"]
        if k["bias"] is not None:
            key = [q for q in sd if q.startswith("mlp_weights.") and q.endswith(".bias")][-1]
            sd[key] = sd[key] + torch.tensor(k["bias"], dtype=torch.float32)
    lv = None
    if k["learn"]:  # entries below, inside and above the clamp [log (0.67 s)^2, log (1.33 s)^2] = log s^2 + [-0.80, 0.57]
        lv = torch.from_numpy((math.log(k["std"] ** 2) + np.random.RandomState(1).uniform(-1.2, 1.2, size=n_lv)).astype(np.float32))
    return sd, dict(O.init_params(crit, 72)), lv


def cfg_of(family, name):
    k = CASES[family][name]
    lo, hi = std_range(k)
    kw = dict(fixed_std=k["std"], learn_fixed_std=k["learn"], std_min=lo, std_max=hi, clip_ploss_coef=CLIP, clip_vloss_coef=k["vclip"],
              norm_adv=k["norm"])
    if family == "gaussian":
        return O.GaussianCfg(tanh_output=k["tanh"], randn_clip_value=3.0, **kw)
    return O.GmmCfg(num_modes=k["M"], **kw)


d64 = lambda p: {q: v.to(F64) for q, v in p.items()}
f32 = lambda t: t.to(torch.float32)


def _targets(lp_cycle, n, top):
    """Per-sample log-prob targets: 'in' spread over the window below `top` (the largest log p the head can give here),
    'above' between the window's upper edge and `top`, 'below' a few nats under the window, 'far' hundreds."""
    out = []
    for i in range(n):
        kind = lp_cycle[i % len(lp_cycle)]
        frac = (i * 0.6180339887) % 1.0
        if kind == "in":
            hi = min(1.6, float(top[i]) - 0.2)
            assert hi > -4.0, "this case cannot reach the window"
            t = -4.4 + frac * (hi + 4.4)
        elif kind == "above":
            assert float(top[i]) > 2.2, "this case cannot reach log p > 2"
            t = 2.0 + (0.3 + 0.5 * frac) * (float(top[i]) - 2.0)
        elif kind == "below":
            t = -6.0 - 3.0 * frac
        else:
            t = -250.0 - 500.0 * frac
        out.append(t)
    return torch.tensor(out, dtype=F64)


def _gmm_logp(means, scales, logits, act):
    comp = (-((act[:, None, :] - means) ** 2) / (2 * scales ** 2) - scales.log() - LOG_SQRT_2PI).sum(-1)
    return torch.logsumexp(torch.log_softmax(logits, -1) + comp, -1)


def _solve_scale(logp_of, target, s_max=80.0, steps=1600):
    """Per sample, the LARGEST s with logp_of(s) = target (log p falls without bound as s grows): grid, then bisection."""
    grid = torch.linspace(0.0, s_max, steps + 1, dtype=F64)
    vals = torch.stack([logp_of(torch.full_like(target, float(s))) for s in grid], 1)  # (B, steps + 1)
    above = vals > target[:, None]
    assert bool(above[:, 0].all()), "a target above the largest log p of its sample"
    assert not bool(above[:, -1].any())
    idx = (above.to(torch.int64) * torch.arange(steps + 1)).max(1).values
    lo, hi = grid[idx], grid[idx + 1]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        up = logp_of(mid) > target
        lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def inputs(family, name):
    """The float32 inputs of one case, max(N, Ni) rows: state, actions (built as the module docstring says), recorded noise
    (and modes), oldlogp, advantages, oldvalues, returns."""
    k = CASES[family][name]
    a, crit = specs(family, name)
    sd, cr, lv = weights(family, name)
    gc = cfg_of(family, name)
    B, AF = max(k["N"], k["Ni"]), k["Ta"] * k["Da"]
    rs = np.random.RandomState(7)
    state = torch.from_numpy(rs.uniform(-1, 1, size=(B, 1, k["cond"])).astype(np.float32))
    u = torch.from_numpy(rs.choice([-1.0, 1.0], size=(B, AF)) * rs.uniform(0.5, 1.5, size=(B, AF)))
    noise = torch.from_numpy((1.6 * rs.randn(B, AF)).astype(np.float32))  # some draws beyond randn_clip_value = 3
    s64, lv64 = state.to(F64), None if lv is None else lv.to(F64)
    with torch.no_grad():
        if family == "gaussian":
            mean, scale = O.gaussian_dist(gc, a, d64(sd), lv64, s64)
            c0 = (-scale.log() - LOG_SQRT_2PI).mean(-1)  # log p at the mean; log p(s) = c0 - s^2 mean(u^2) / 2
            target = _targets(k["lp"], B, c0)
            s = torch.sqrt(2 * (c0 - target) / (u * u).mean(-1))
            actions = mean + scale * s[:, None] * u
            modes = None
        else:
            means, scales, logits = O.gmm_dist(gc, a[0], a[1], d64(sd), lv64, s64, k["Da"], k["Ta"])
            rows = torch.arange(B)
            modes = torch.from_numpy(rs.randint(0, k["M"], size=B).astype(np.int64))  # the recorded draws of the sampling test
            if k["far"]:
                actions = 2.0 * torch.sign(u)
            else:  # the action of sample i leaves the mean of component home[i] (one the mixture has not switched off)
                live = [j for j in range(k["M"]) if k["bias"] is None or k["bias"][j] > -1.0]
                home = torch.tensor([live[(3 * j) % len(live)] for j in range(B)])
                of = lambda sc: _gmm_logp(means, scales, logits, means[rows, home] + scales[rows, home] * sc[:, None] * u)
                target = _targets(k["lp"], B, of(torch.zeros(B, dtype=F64)))
                actions = means[rows, home] + scales[rows, home] * _solve_scale(of, target)[:, None] * u
        actions = f32(actions)
        if family == "gaussian":
            logp = O.gaussian_logprob(gc, a, d64(sd), lv64, s64, actions.to(F64))[0]
        else:
            logp = O.gmm_logprob(gc, a[0], a[1], d64(sd), lv64, s64, actions.to(F64), k["Da"], k["Ta"])[0]
        v = O.critic_forward(d64(cr), crit, s64).view(-1)
    i = torch.arange(B)
    oldlogp = logp.clamp(-5, 2) + torch.tensor(OFF, dtype=F64)[i % 4]
    oldlogp[i % 11 == 5] = 2.7  # a few old log-probs beyond the window themselves, on each side
    oldlogp[i % 11 == 8] = -6.5
    adv = torch.tensor(ADV, dtype=F64)[i % 7]
    oldv = v + torch.tensor(OLDV, dtype=F64)[i % 4]
    ret = v + torch.tensor(RET, dtype=F64)[i % 3]
    return dict(state=state, actions=actions, noise=noise, modes=modes, oldlogp=f32(oldlogp), adv=f32(adv), oldvalues=f32(oldv),
                returns=f32(ret))


# --------------------------------------------------------------------------------------------------- float64 reference
def _stats(res):
    return np.array([res[0].item(), res[1].item(), res[2].item(), res[3], res[4], res[5], float(res[6]), res[7]])


@functools.lru_cache(maxsize=None)
def reference(family, name):
    """Everything the GPU tests compare against, computed once per case in float64 and never modified: sampled actions (recorded
    draws; deterministic), log-probs, the PPO loss 8-tuple with the gradients of pg + ENT_COEF entropy_loss + 0.5 v over the first
    N rows, the BC loss / entropy with its gradients over the first Ni rows, and the critic's values."""
    k = CASES[family][name]
    a, crit = specs(family, name)
    sd, cr, lv = weights(family, name)
    gc = cfg_of(family, name)
    x = inputs(family, name)
    N, Ni, Da, Ta = k["N"], k["Ni"], k["Da"], k["Ta"]
    S = x["state"].to(F64)
    A = x["actions"].to(F64)
    gmm = family == "gmm"

    def leaves():
        p = {q: t.to(F64).clone().requires_grad_(True) for q, t in sd.items()}
        c = {q: t.to(F64).clone().requires_grad_(True) for q, t in cr.items()}
        l = None if lv is None else lv.to(F64).clone().requires_grad_(True)
        return p, c, l

    def grads(p, c, l):
        g = {q: t.grad.detach().clone() for q, t in p.items() if t.grad is not None}
        g.update({"critic." + q: t.grad.detach().clone() for q, t in c.items() if t.grad is not None})
        if l is not None:
            g["logvar"] = l.grad.detach().clone()
        return g

    out = {}
    p, c, l = leaves()
    with torch.no_grad():
        if gmm:
            out["sample"] = O.gmm_sample(gc, a[0], a[1], p, l, S[:Ni], x["modes"][:Ni], x["noise"][:Ni].to(F64), Da, Ta)
            means = O.gmm_dist(gc, a[0], a[1], p, l, S[:Ni], Da, Ta)[0]
            out["sample_det"] = (means[torch.arange(Ni), x["modes"][:Ni]] + 1e-4 * x["noise"][:Ni].to(F64)).view(Ni, Ta, Da)
            out["logp"] = O.gmm_logprob(gc, a[0], a[1], p, l, S, A, Da, Ta)[0]
        else:
            out["sample"] = O.gaussian_sample(gc, a, p, l, S[:Ni], x["noise"][:Ni].to(F64))
            out["sample_det"] = O.gaussian_sample(gc, a, p, l, S[:Ni], x["noise"][:Ni].to(F64), deterministic=True)
            out["logp"] = O.gaussian_logprob(gc, a, p, l, S, A)[0]
        out["v"] = O.critic_forward(c, crit, S).view(-1)
    r = lambda key: x[key][:N].to(F64)
    if gmm:
        res = O.gmm_ppo_loss(gc, a[0], a[1], crit, p, l, c, S[:N], A[:N], r("returns"), r("oldvalues"), r("adv"), r("oldlogp"), Da, Ta)
    else:
        res = O.gaussian_ppo_loss(gc, a, crit, p, l, c, S[:N], A[:N], r("returns"), r("oldvalues"), r("adv"), r("oldlogp"))
    out["stats"] = _stats(res)
    (res[0] + ENT_COEF * res[1] + 0.5 * res[2]).backward()
    out["ppo_grads"] = grads(p, c, l)
    p, c, l = leaves()
    if gmm:
        lp, ent, _ = O.gmm_logprob(gc, a[0], a[1], p, l, S[:Ni], A[:Ni], Da, Ta)
        loss = -lp.mean()
    else:
        mean, scale = O.gaussian_dist(gc, a, p, l, S[:Ni])
        dist = torch.distributions.Normal(mean, scale)
        ent = dist.entropy().mean()
        loss = -dist.log_prob(A[:Ni]).mean() - BC_ENT_COEF * ent
    loss.backward()
    out["bc"] = (loss.item(), ent.item())
    out["bc_grads"] = grads(p, c, l)
    return out


def clamp_mask(family, name):
    """True where a logvar entry lies OUTSIDE the clamp range (float64 bounds), and each entry's distance to the nearer end."""
    k = CASES[family][name]
    lv = weights(family, name)[2].to(F64)
    lo, hi = (math.log(s ** 2) for s in std_range(k))
    return ((lv < lo) | (lv > hi)).numpy(), torch.minimum((lv - lo).abs(), (lv - hi).abs()).numpy(), (lv < lo).numpy(), (lv > hi).numpy()


def regimes_and_margins(family, name):
    """(set of regime names populated by the first N rows, [(what, sample, distance, band)] of every float32 decision)."""
    k = CASES[family][name]
    x, ref = inputs(family, name), reference(family, name)
    N = k["N"]
    logp, old = ref["logp"][:N], x["oldlogp"][:N].to(F64)
    adv = x["adv"][:N].to(F64)
    if k["norm"]:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = (logp.clamp(-5, 2) - old.clamp(-5, 2)).exp()
    lo, hi = 1 - CLIP, 1 + CLIP
    got, margins = set(), []
    blp, bv = BAND_LP[family], BAND_V[family]
    for i in range(N):
        l, o, r, ad = float(logp[i]), float(old[i]), float(ratio[i]), float(adv[i])
        got.add("logp_far" if l < -100 else "logp_below" if l < -5 else "logp_above" if l > 2 else "logp_in")
        if o > 2 or o < -5:
            got.add("old_above" if o > 2 else "old_below")
        got.add(("ratio_lo" if r < lo else "ratio_hi" if r > hi else "ratio_in") + ("_adv+" if ad > 0 else "_adv-"))
        margins += [("logp|2", i, abs(l - 2), blp), ("logp|-5", i, abs(l + 5), blp), ("old|2", i, abs(o - 2), blp),
                    ("old|-5", i, abs(o + 5), blp), ("ratio|lo", i, abs(r - lo), blp * max(r, 1.0)),
                    ("ratio|hi", i, abs(r - hi), blp * max(r, 1.0)), ("adv|0", i, abs(ad), BAND_ADV)]
        if k["vclip"] is not None:
            v, ov, ret = float(ref["v"][i]), float(x["oldvalues"][i]), float(x["returns"][i])
            dlt = v - ov
            active = abs(dlt) > CV
            margins.append(("dv|cv", i, abs(abs(dlt) - CV), bv * max(1.0, abs(v))))
            if active:  # (inactive: vc = v, lu = lc up to rounding, and both branches give the same gradient)
                vc = ov + max(-CV, min(CV, dlt))
                lu, lc = (v - ret) ** 2, (vc - ret) ** 2
                got.add("vclip_active_lu>lc" if lu > lc else "vclip_active_lu<lc")
                margins.append(("lu|lc", i, abs(lu - lc), bv * max(1.0, lu, lc)))
            else:
                got.add("vclip_inactive")
    if k["learn"]:
        out, dist, below, above = clamp_mask(family, name)
        got |= {n for n, m in (("logvar_below", below), ("logvar_above", above), ("logvar_inside", ~out)) if m.any()}
        margins += [("logvar|clamp", j, float(d), BAND_LOGVAR) for j, d in enumerate(dist)]
    return got, margins


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_case_lists_cover_the_shapes_and_switches():
    """Every shape and switch listed below appears at least once per family (every case runs all four kernels), and every ragged N
    is paired with a learned std at least once -- only then do dead rows touch shared memory."""
    g, m = GAUSS.values(), GMM.values()
    assert {k["N"] for k in g} == {2, 15, 16, 17, 33} and {k["Ni"] for k in g} == {1, 17}
    assert {(k["Ta"], k["Da"]) for k in g} == {(1, 1), (3, 5), (4, 4), (1, 17), (2, 20)}
    for key in ("tanh", "learn", "norm"):
        assert {k[key] for k in g} == {True, False}
    assert {k["vclip"] for k in g} == {None, CV} == {k["vclip"] for k in m}
    assert {k["N"] for k in m} == {2, 3, 4, 5, 9} and {k["Ni"] for k in m} == {1, 5}
    assert {(k["M"], k["Ta"], k["Da"]) for k in m} == {(1, 1, 1), (8, 1, 8), (5, 1, 13), (2, 4, 2), (8, 3, 7)}
    assert {k["M"] * k["Ta"] * k["Da"] for k in m} >= {1, 64, 65, 168}
    assert {k["learn"] for k in m} == {True, False} == {k["res"] for k in m}
    assert {k["N"] for k in g if k["learn"]} >= {2, 15, 17, 33} and {k["Ni"] for k in g if k["learn"]} == {1, 17}
    assert {k["N"] for k in m if k["learn"]} >= {2, 3, 5, 9} and {k["Ni"] for k in m if k["learn"]} == {1, 5}
    assert any(k["bias"] for k in m) and any(k["far"] for k in m)


@pytest.mark.parametrize("fc", ALL, ids=ids)
def test_cases_populate_every_regime_and_no_sample_is_fragile(fc):
    """On the float64 oracle alone: the regimes HOME assigns to this case are populated, every log-prob target was met, and every
    sample is at least its guard band away from every decision the kernel takes in float32 (the window edges of logp and
    oldlogp, ratio against 1 -+ clip, v - oldv against +-cv, lu against lc, each logvar entry against the clamp ends)."""
    family, name = fc
    k = CASES[family][name]
    got, margins = regimes_and_margins(family, name)
    want = {r for r, home in HOME[family].items() if home == name}
    print(f"{family} {name}: regimes {sorted(got)}")
    assert want <= got, sorted(want - got)
    fragile = [m for m in margins if not m[2] >= m[3]]
    assert not fragile, fragile
    ref = reference(family, name)
    assert all(np.isfinite(ref["stats"])) and bool(torch.isfinite(ref["logp"]).all())
    kinds = {"in": "logp_in", "above": "logp_above", "below": "logp_below", "far": "logp_far"}
    assert {kinds[c] for i, c in zip(range(k["N"]), k["lp"] * 40)} <= got
    if k.get("far"):
        assert float(ref["logp"].max()) < -200  # every component log-density hundreds of nats below zero
    if k.get("bias"):
        sd = weights(family, name)[0]
        a, _ = specs(family, name)
        x = inputs(family, name)
        logits = O.gmm_dist(cfg_of(family, name), a[0], a[1], d64(sd), None, x["state"].to(F64), k["Da"], k["Ta"])[2]
        pi = logits.softmax(-1)
        assert float(pi[:, 2].max()) < 1e-40 and float(pi[:, 1].max()) < 1e-12 and float(pi[:, 0].min()) > 0.1  # underflows in fp32
    if k["learn"]:
        out = clamp_mask(family, name)[0]
        assert not ref["ppo_grads"]["logvar"].numpy()[out].any() and not ref["bc_grads"]["logvar"].numpy()[out].any()
        assert ref["ppo_grads"]["logvar"].numpy()[~out].all()  # ... and the entries the clamp passes do get a gradient


def test_every_regime_has_a_home():
    for family in CASES:
        assert set(HOME[family].values()) <= set(CASES[family])
        union = set().union(*(regimes_and_margins(family, n)[0] for n in CASES[family]))
        assert union == set(HOME[family]), union ^ set(HOME[family])


def _ppo_fixture(learn):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.common.mlp_gmm import GMM_MLP
    wide = Gaussian_MLP(action_dim=100, horizon_steps=8, cond_dim=4, mlp_dims=[256, 256, 256], residual_style=True, fixed_std=0.1,
                        learn_fixed_std=learn, precision="fp32")
    gmm = GMM_MLP(action_dim=65, horizon_steps=1, cond_dim=4, mlp_dims=[256, 256], num_modes=8, activation_type="ReLU",
                  residual_style=False, fixed_std=0.1, learn_fixed_std=learn, precision="fp32")
    critic = CriticObs(cond_dim=4, mlp_dims=[256, 256, 256], activation_type="Mish", residual_style=True, precision="fp32")
    return wide, gmm, critic


def test_ppo_entries_refuse_what_the_bc_entries_refuse_on_the_host():
    """dppo_gmm_ppo_loss_fwd_bwd at M = 8, Ta = 1, Da = 65 (each block's row of partials is 8 + 520 doubles, the workspace
    reserves 8 + 8 * 64) and dppo_gaussian_ppo_loss_fwd_bwd at a learned std with Ta * Da = 800 (16 * 800 floats of dynamic
    shared memory: the launch would fail): -1 with the BC entries' messages, before the first launch -- every pointer is the
    dummy address 4096."""
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch
    err = lambda: lib.dppo_last_error().decode()
    N = 64
    for learn in (False, True):
        wide, gmm, critic = _ppo_fixture(learn)
        dc = critic.net_desc()
        m, w = gmm._trunks(bind=False)
        dm, dw, cfg = m.net_desc(), w.net_desc(), gmm.gmm_cfg()
        ws = lib.dppo_gmm_workspace_bytes(C.byref(dm), C.byref(dw), C.byref(dc), hip.PREC_F32, N)
        assert ws > 0, err()
        rc = lib.dppo_gmm_ppo_loss_fwd_bwd(C.byref(dm), C.byref(dw), C.byref(dc), hip.PREC_F32, X, X, X, X, X, X, C.byref(cfg), X, X, X,
                                           X, X, X, X, N, None, X, X, X, X, X, X, ws, None)
        assert rc == -1 and "action_dim above 64" in err(), (rc, err())
        da, gcfg = wide.net_desc(), wide.gaussian_cfg()
        ws = lib.dppo_gaussian_workspace_bytes(C.byref(da), C.byref(dc), hip.PREC_F32, N)
        assert ws > 0, err()
        if learn:  # (a fixed std keeps nothing in shared memory: Ta * Da = 800 is served, so it is not called with dummies)
            rc = lib.dppo_gaussian_ppo_loss_fwd_bwd(C.byref(da), C.byref(dc), hip.PREC_F32, X, X, X, X, C.byref(gcfg), X, X, X, X, X, X,
                                                    X, N, None, X, X, X, X, X, ws, None)
            assert rc == -1 and "above 768" in err(), (rc, err())
            # the refusals the PPO entries had before still come first / still hold
            rc = lib.dppo_gaussian_ppo_loss_fwd_bwd(C.byref(da), C.byref(dc), hip.PREC_F32, X, X, X, X, C.byref(gcfg), X, X, X, X, X, X,
                                                    X, N, None, X, X, None, X, X, ws, None)
            assert rc == -1 and "needs logvar_grad" in err(), (rc, err())


# ------------------------------------------------------------------------------------------------------------------- GPU
def _last_bias(keys, prefix):
    return [q for q in keys if q.startswith(prefix) and q.endswith(".bias")][-1]


def build_model(family, name, prec):
    from dppo_amd.model.common.critic import CriticObs
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.common.mlp_gmm import GMM_MLP
    from dppo_amd.model.rl.gaussian_ppo import PPO_Gaussian
    from dppo_amd.model.rl.gmm_ppo import PPO_GMM
    k = CASES[family][name]
    sd, cr, lv = weights(family, name)
    sd = dict(sd)
    lo, hi = std_range(k)
    kw = dict(action_dim=k["Da"], horizon_steps=k["Ta"], cond_dim=k["cond"], activation_type=k["act"], fixed_std=k["std"],
              learn_fixed_std=k["learn"], std_min=lo, std_max=hi, precision=prec)
    if lv is not None:
        sd["logvar"] = lv
    if family == "gaussian":
        actor = Gaussian_MLP(mlp_dims=list(TRUNK), tanh_output=k["tanh"], residual_style=True, **kw)
        actor.load_state_dict(sd, strict=False)
    else:
        actor = GMM_MLP(mlp_dims=list(TRUNK) if k["res"] else [64, 64], num_modes=k["M"], residual_style=k["res"], **kw)
        sd["logvar_min"], sd["logvar_max"] = actor.logvar_min.data.clone(), actor.logvar_max.data.clone()
        actor.load_state_dict(sd, strict=True)
    critic = CriticObs(cond_dim=k["cond"], mlp_dims=list(TRUNK), activation_type="Mish", residual_style=True, precision=prec)
    critic.load_state_dict(cr, strict=True)
    kw = dict(actor=actor, critic=critic, horizon_steps=k["Ta"], device="cuda:0", clip_ploss_coef=CLIP, clip_vloss_coef=k["vclip"],
              norm_adv=k["norm"])
    if family == "gaussian":
        return PPO_Gaussian(randn_clip_value=3.0, **kw)
    m = PPO_GMM(precision=prec, **kw)
    m.ent_coef = ENT_COEF  # the entropy term's gradient rides pg_loss
    return m


@functools.lru_cache(maxsize=None)
def fp32_model(family, name):
    return build_model(family, name, "fp32")


def dev_inputs(family, name, n):
    x = inputs(family, name)
    return {q: (None if t is None else t[:n].contiguous().cuda()) for q, t in x.items()}


def zero_grads(m):
    for p in list(m.actor_ft.parameters()) + list(m.critic.parameters()):
        p.grad = None


def named_grads(m, with_critic=True):
    out = {q: p.grad.double().cpu() for q, p in m.actor_ft.named_parameters() if p.grad is not None}
    if with_critic:
        out.update({"critic." + q: p.grad.double().cpu() for q, p in m.critic.named_parameters() if p.grad is not None})
    return out


def rel_close(got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| per element; log-probs of magnitude 1e2 .. 1e3 are thereby compared relatively."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    return float(err.max()), bool((err <= 1.0).all())


VANISHING = 1e-12  # a float64 reference gradient norm below this is the roundoff of an analytic zero (real ones are 1e-3 .. 1e2)


def check_grads(family, got, ref, out_mask, label):
    """logvar: EXACT zeros at the clamped entries, both families.

    Gaussian (tests/test_gaussian.py's bound, rtol 2e-3 and atol 2e-6 per element): logvar and the output-layer biases of the
    trunk and of the critic (the column sums of d_mean / d_v: the head's own output, no GEMM in between) per element, every
    tensor by ||g - ref|| <= 2e-3 ||ref|| + 2e-6 sqrt(size).

    Mixture (tests/test_gmm.py's bounds, as ``grad_report`` measures them): actor (both trunks and logvar) and critic are one
    group each.  Every tensor carrying >= 1e-6 of its group's squared reference norm: ||g - ref|| < rtol ||ref||, rtol 1e-2
    for the actor and 5e-3 for the critic, nothing added.  The group's norm: |sqrt(n_got / n_ref) - 1| < 2e-3 / 1e-3.  A tensor
    under that share -- grad_report skips it -- is held to floor = rtol * 1e-3 * the group's norm, the error a tensor at the
    cutoff is allowed.  logvar and the output-layer biases (column sums of d_mean / d_logits / d_v) also per element:
    |g - ref| <= max(rtol |ref|, floor) -- an element is held to rtol of itself; the floor only takes over where the element is
    under 1e-3 of the group's norm, such as a column whose terms cancel (N = 2, dv = -+0.3: the critic's output bias sums to 0).
    A group whose reference norm is under VANISHING has no reference to be relative to: with a fixed std and every log p
    outside the window the actor's gradient is coef = 0 times the likelihood term plus ent_coef / N * pi_m (H_m - Hbar) with all
    H_m equal.  fp32 leaves a residual of at most a few ulp (6e-8) of ent_coef / N * H = 0.002 * 30 per logit, under 1e-7 in
    norm after the trunk's backward; the smallest real term (one H_m off by 0.1) is 1e-4.  Such a group is held to ||g|| <= 1e-6."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    if out_mask is not None:
        assert not got["logvar"].numpy()[out_mask].any() and not ref["logvar"].numpy()[out_mask].any(), (label, got["logvar"], out_mask)
    biases = {_last_bias(ref, "mlp_mean.")} | ({_last_bias(ref, "mlp_weights.")} if family == "gmm" else set())
    if any(q.startswith("critic.") for q in ref):
        biases.add(_last_bias(ref, "critic."))
    flat = lambda t: t.reshape(-1).numpy()
    worst = {}
    if family == "gaussian":
        for q, r in ref.items():
            g, r = flat(got[q]), flat(r)
            if q == "logvar" or q in biases:
                e, ok = rel_close(g, r, 2e-3, 2e-6)
                worst["element / bound"] = max(worst.get("element / bound", (0.0, "")), (e, q))
                assert ok, (label, q, e, g, r)
            err, bound = float(np.linalg.norm(g - r)), 2e-3 * float(np.linalg.norm(r)) + 2e-6 * math.sqrt(r.size)
            worst["tensor / bound"] = max(worst.get("tensor / bound", (0.0, "")), (err / bound, q))
            assert err <= bound, (label, q, err, bound)
        print(f"  {label}: worst gradient errors {worst}")
        return
    for group, rtol, ntol in (("actor", 1e-2, 2e-3), ("critic", 5e-3, 1e-3)):
        keys = [q for q in ref if q.startswith("critic.") == (group == "critic")]
        if not keys:
            continue
        n_ref = sum(float(np.dot(flat(ref[q]), flat(ref[q]))) for q in keys)
        n_got = sum(float(np.dot(flat(got[q]), flat(got[q]))) for q in keys)
        if math.sqrt(n_ref) < VANISHING:
            worst[group + " vanishing, ||g||"] = math.sqrt(n_got)
            assert math.sqrt(n_got) <= 1e-6, (label, group, n_got)
            continue
        floor = rtol * 1e-3 * math.sqrt(n_ref)
        nerr = abs(math.sqrt(n_got / n_ref) - 1.0)
        worst[group + " norm error"] = nerr
        assert nerr < ntol, (label, group, nerr)
        for q in keys:
            g, r = flat(got[q]), flat(ref[q])
            err, nr = float(np.linalg.norm(g - r)), float(np.linalg.norm(r))
            if nr * nr >= 1e-6 * n_ref:
                worst[group + " tensor"] = max(worst.get(group + " tensor", (0.0, "")), (err / nr, q))
                assert err < rtol * nr, (label, q, err / nr)
            else:
                worst[group + " small tensor / floor"] = max(worst.get(group + " small tensor / floor", (0.0, "")), (err / floor, q))
                assert err <= floor, (label, q, err, floor)
            if q == "logvar" or q in biases:
                e = np.abs(g - r) / np.maximum(rtol * np.abs(r), floor)
                worst[group + " element / bound"] = max(worst.get(group + " element / bound", (0.0, "")), (float(e.max()), q))
                assert (e <= 1.0).all(), (label, q, float(e.max()), g, r)
    print(f"  {label}: worst gradient errors {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("fc", ALL, ids=ids)
def test_hip_sampling_and_logprobs(fc):
    """Ni = 1 / 17 (Gaussian) or 1 / 5 (mixture) rows: actions with the recorded noise (and modes), the deterministic draw
    (sigma = 1e-4: the means), and the per-sample log-probs -- magnitudes up to 1e3 -- against float64."""
    family, name = fc
    k = CASES[family][name]
    m, ref, x = fp32_model(family, name), reference(family, name), dev_inputs(family, name, CASES[family][name]["Ni"])
    cond = {"state": x["state"]}
    extra = dict(modes=x["modes"]) if family == "gmm" else {}
    act = m(cond=cond, deterministic=False, noise=x["noise"], **extra)
    det = m(cond=cond, deterministic=True, noise=x["noise"], **extra)
    tol = TOL[family]["act"]
    assert tuple(act.shape) == (k["Ni"], k["Ta"], k["Da"])
    np.testing.assert_allclose(act.cpu().numpy(), ref["sample"].numpy(), rtol=tol, atol=tol)
    np.testing.assert_allclose(det.cpu().numpy(), ref["sample_det"].numpy(), rtol=tol, atol=tol)
    lp = m.get_logprobs(cond, x["actions"])[0]
    e, ok = rel_close(lp.cpu().numpy(), ref["logp"][:k["Ni"]].numpy(), TOL[family]["lp"], TOL[family]["lp"])
    print(f"{family} {name}: log-prob error / tolerance {e:.3f}")
    assert ok, (lp.cpu().numpy(), ref["logp"][:k["Ni"]].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("fc", ALL, ids=ids)
def test_hip_ppo_loss_statistics_and_every_gradient(fc):
    """N = 2 .. 33 (Gaussian) / 2 .. 9 (mixture): the loss 8-tuple and the gradients of pg + 0.01 entropy_loss + 0.5 v -- logvar
    with exact zeros at the clamped entries, the output-layer biases per element, every other tensor by its norm -- and the
    log-probs of all N rows through the logprob kernel."""
    family, name = fc
    k = CASES[family][name]
    m, ref, x = fp32_model(family, name), reference(family, name), dev_inputs(family, name, CASES[family][name]["N"])
    cond = {"state": x["state"]}
    lp = m.get_logprobs(cond, x["actions"])[0]
    e, ok = rel_close(lp.cpu().numpy(), ref["logp"][:k["N"]].numpy(), TOL[family]["lp"], TOL[family]["lp"])
    assert ok, (lp.cpu().numpy(), ref["logp"][:k["N"]].numpy())
    zero_grads(m)
    res = m.loss(cond, x["actions"], x["returns"], x["oldvalues"], x["adv"], x["oldlogp"])
    got = _stats(res)
    rtol, atol = TOL[family]["stat"]
    print(f"{family} {name}: log-prob error / tolerance {e:.3f}; stats {got.tolist()} ref {ref['stats'].tolist()}")
    np.testing.assert_allclose(got, ref["stats"], rtol=rtol, atol=atol)
    assert abs(got[3] - ref["stats"][3]) < 0.25 / k["N"]  # clipfrac counts samples (the oracle's mean is a float32): the same count
    if family == "gaussian":
        (res[0] + ENT_COEF * res[1] + 0.5 * res[2]).backward()
    else:
        (res[0] + 0.5 * res[2]).backward()  # model.ent_coef: the entropy's gradient is already in pg_loss's
    out = clamp_mask(family, name)[0] if k["learn"] else None
    check_grads(family, named_grads(m), ref["ppo_grads"], out, f"{family} {name} ppo")
    zero_grads(m)


@pytest.mark.gpu
@pytest.mark.parametrize("fc", ALL, ids=ids)
def test_hip_bc_loss_entropy_and_every_gradient(fc):
    """GaussianModel.loss (ent_coef 0.05) / GMMModel.loss on Ni rows: loss, entropy and every gradient, logvar's with exact zeros
    at the clamped entries (likelihood and entropy bonus).  The mixture's *far* case has every component log-density hundreds
    of nats below zero, the *bias* case mixture weights that underflow to 0."""
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.gmm import GMMModel
    family, name = fc
    k = CASES[family][name]
    m, ref, x = fp32_model(family, name), reference(family, name), dev_inputs(family, name, CASES[family][name]["Ni"])
    cond = {"state": x["state"]}
    zero_grads(m)
    if family == "gaussian":
        loss, info = GaussianModel.loss(m, x["actions"], cond, BC_ENT_COEF)
    else:
        loss, info = GMMModel.loss(m, x["actions"], cond)
    got = (float(loss.detach()), float(info["entropy"]))
    rtol, atol = TOL[family]["stat"]
    print(f"{family} {name}: bc loss / entropy {got} ref {ref['bc']}")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref["bc"], rtol=rtol, atol=atol)
    loss.backward()
    out = clamp_mask(family, name)[0] if k["learn"] else None
    check_grads(family, named_grads(m, with_critic=False), ref["bc_grads"], out, f"{family} {name} bc")
    zero_grads(m)


SENTINEL = 12345.0


@pytest.mark.gpu
@pytest.mark.parametrize("fc", [("gaussian", "n17_1x17_learn_notanh"), ("gaussian", "n33_2x20_learn"), ("gmm", "n9_m8_3x7_learn"),
                                ("gmm", "n5_m2_4x2_learn")], ids=ids)
def test_hip_inference_kernels_write_nothing_past_row_n(fc):
    """dppo_*_sample / dppo_*_logprob through the C ABI at ragged N (17; 5), the outputs being the front of a larger
    sentinel-filled tensor: the sentinel behind element N * Ta * Da (actions, means) or N (log-probs) is intact, and the
    front holds what the model call returns."""
    from dppo_amd import hip
    family, name = fc
    k = CASES[family][name]
    m, x = fp32_model(family, name), dev_inputs(family, name, CASES[family][name]["Ni"])
    lib, net = hip.load(), m.actor_ft
    n, AF, dev = k["Ni"], k["Ta"] * k["Da"], "cuda:0"
    assert n % (16 if family == "gaussian" else 4)
    obs = x["state"].reshape(n, -1).contiguous()
    big = lambda: torch.full((n * AF + 4096,), SENTINEL, device=dev)
    act, mean, logp = big(), big(), big()
    cond = {"state": x["state"]}
    if family == "gaussian":
        d, cfg = net.net_desc(), net.gaussian_cfg(randn_clip=3.0)
        wsb = lib.dppo_gaussian_workspace_bytes(C.byref(d), None, m.prec, n)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        head = (C.byref(d), m.prec, net.flat_params().data_ptr(), net.packed(m.prec, 0).data_ptr(), C.byref(cfg), net.logvar_ptr(),
                obs.data_ptr())
        hip.check(lib.dppo_gaussian_sample(*head, x["noise"].data_ptr(), n, act.data_ptr(), mean.data_ptr(), ws.data_ptr(), wsb,
                                           hip.stream()), "dppo_gaussian_sample")
        hip.check(lib.dppo_gaussian_logprob(*head, x["actions"].data_ptr(), n, logp.data_ptr(), ws.data_ptr(), wsb, hip.stream()),
                  "dppo_gaussian_logprob")
        assert bool((mean[n * AF:] == SENTINEL).all()) and not bool((mean[:n * AF] == SENTINEL).any())
        want = m(cond=cond, noise=x["noise"])
    else:
        mn, wn = net.mean_net, net.weights_net
        cfg = net.gmm_cfg()
        wsb = lib.dppo_gmm_workspace_bytes(C.byref(mn.net_desc()), C.byref(wn.net_desc()), None, m.prec, n)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        head = (*m._net_args(net), C.byref(cfg), net.logvar_ptr(), obs.data_ptr())
        hip.check(lib.dppo_gmm_sample(*head, x["modes"].data_ptr(), x["noise"].data_ptr(), n, act.data_ptr(), ws.data_ptr(), wsb,
                                      hip.stream()), "dppo_gmm_sample")
        hip.check(lib.dppo_gmm_logprob(*head, x["actions"].data_ptr(), n, logp.data_ptr(), ws.data_ptr(), wsb, hip.stream()),
                  "dppo_gmm_logprob")
        want = m(cond=cond, modes=x["modes"], noise=x["noise"])
    torch.cuda.synchronize()
    assert bool((act[n * AF:] == SENTINEL).all()) and bool((logp[n:] == SENTINEL).all())
    assert torch.equal(act[:n * AF], want.reshape(-1)) and torch.equal(logp[:n], m.get_logprobs(cond, x["actions"])[0])


@pytest.mark.gpu
def test_hip_gmm_shards_with_pooled_moments_add_up():
    """The data-parallel contract of PPO_GMM.ppo_update(global_moments=...): N = 9 evaluated as shards of 5 and 4 with the pooled
    advantage moments -- the gradients of both trunks, the critic and logvar (entropy term included) and the five summed
    statistics add up to the whole's, within the bounds tests/test_gaussian.py holds the Gaussian head to."""
    family, name = "gmm", "n9_m8_3x7_learn"
    m, x = fp32_model(family, name), dev_inputs(family, name, 9)
    N = 9
    args = tuple(x[q].reshape(N, -1).contiguous() if q in ("state", "actions") else x[q]
                 for q in ("state", "actions", "returns", "oldvalues", "adv", "oldlogp"))
    st = m.ppo_update(*args).cpu().numpy().copy()
    net = m.actor_ft
    ga, gc, gl = net.flat_grads().double().clone(), m.critic.flat_grads().double().clone(), m._lv_grad.double().clone()
    n_mean = net.mean_net.flat_params().numel()
    assert float(ga[:n_mean].norm()) > 0 and float(ga[n_mean:].norm()) > 0 and float(gl.norm()) > 0 and float(gc.norm()) > 0
    am = args[4].double()
    gm = torch.stack([am.sum(), (am * am).sum(), torch.tensor(float(N), dtype=torch.float64, device=am.device)])
    sa, sc, sl, ss = torch.zeros_like(ga), torch.zeros_like(gc), torch.zeros_like(gl), np.zeros(5)
    for lo, hi in ((0, 5), (5, 9)):
        s2 = m.ppo_update(*(t[lo:hi].contiguous() for t in args), global_moments=gm).cpu().numpy()
        sa += net.flat_grads().double()
        sc += m.critic.flat_grads().double()
        sl += m._lv_grad.double()
        ss += s2[:5]  # each shard already divides by the global count
    for got, whole in ((sa[:n_mean], ga[:n_mean]), (sa[n_mean:], ga[n_mean:]), (sc, gc)):
        assert (got - whole).norm().item() <= 2e-5 * whole.norm().item()
    assert (sl - gl).norm().item() <= 1e-4 * gl.norm().item() + 1e-12
    out = clamp_mask(family, name)[0]
    assert not sl.cpu().numpy()[out].any() and not gl.cpu().numpy()[out].any()
    np.testing.assert_allclose(ss, st[:5], rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("fc", RAGGED_LEARNED, ids=ids)
def test_hip_bf16_ragged_learned_std(fc):
    """bf16 operands on the ragged-N, learned-std cases: every output finite, the log-probs and v_loss within the bf16 bounds of
    tests/test_gaussian.py (0.3 relative + 0.3 absolute; v_loss 5e-2 relative) / tests/test_gmm.py (0.15 absolute; v_loss
    5e-2 relative + 1e-3), and the clamped logvar entries' gradient still exactly zero (PPO and BC)."""
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.gmm import GMMModel
    family, name = fc
    k = CASES[family][name]
    m, ref, x = build_model(family, name, "bf16"), reference(family, name), dev_inputs(family, name, CASES[family][name]["N"])
    bc = dev_inputs(family, name, k["Ni"])
    cond = {"state": x["state"]}
    out = clamp_mask(family, name)[0]
    lp = m.get_logprobs(cond, x["actions"])[0].cpu().numpy()
    want = ref["logp"][:k["N"]].numpy()
    print(f"{family} {name} bf16: log-prob errors {np.abs(lp - want).tolist()} of {want.tolist()}")
    assert np.isfinite(lp).all()
    if family == "gaussian":
        np.testing.assert_allclose(lp, want, rtol=0.3, atol=0.3)
    else:
        assert float(np.abs(lp - want).max()) < 0.15
    act = m(cond=cond, noise=x["noise"], **(dict(modes=x["modes"]) if family == "gmm" else {}))
    assert bool(torch.isfinite(act).all())
    res = m.loss(cond, x["actions"], x["returns"], x["oldvalues"], x["adv"], x["oldlogp"])
    got = _stats(res)
    print(f"  stats {got.tolist()} ref {ref['stats'].tolist()}")
    assert np.isfinite(got).all()
    assert abs(got[2] - ref["stats"][2]) <= 5e-2 * abs(ref["stats"][2]) + (1e-3 if family == "gmm" else 0.0)
    (res[0] + 0.5 * res[2]).backward()
    g = named_grads(m)
    assert all(bool(torch.isfinite(t).all()) for t in g.values())
    assert not g["logvar"].numpy()[out].any() and g["logvar"].numpy()[~out].all()
    zero_grads(m)
    bc_cond, bc_act = {"state": bc["state"]}, bc["actions"]
    loss, info = GaussianModel.loss(m, bc_act, bc_cond, BC_ENT_COEF) if family == "gaussian" else GMMModel.loss(m, bc_act, bc_cond)
    loss.backward()
    g = named_grads(m, with_critic=False)
    assert np.isfinite(float(loss.detach())) and np.isfinite(float(info["entropy"])) and all(bool(torch.isfinite(t).all()) for t in g.values())
    assert not g["logvar"].numpy()[out].any() and g["logvar"].numpy()[~out].all()
