"""Behaviour-cloning pre-training of the Gaussian / mixture-of-Gaussians policies (reference model/common/gaussian.py:49-65,
model/common/gmm.py:40-86, agent/pretrain/train_gaussian_agent.py): the shipped pre_gaussian_mlp / pre_gmm_mlp cfgs resolve (CPU),
the two C ABI entries check their arguments (CPU), and on the GPU ``GaussianModel.loss`` / ``GMMModel.loss`` reproduce the
reference's loss, entropy and every gradient (g22 / g23 fixtures, tests/golden/make_golden_bc.py), the gradients of two half
batches add up to the whole batch's, and a short run's checkpoint feeds the PPO fine-tuning models.

bf16 bounds.  The project had no number for this loss in bf16, so they are measured (profiles/bc_gaussian_parity.json, DESIGN
section 14): per case, against the REFERENCE golden,
  loss error       |loss - ref| / max(1, |ref|)  (the losses run from -37 to +408 and cross zero, so the floor of the fp32 check),
  gradient error   worst per-tensor ||g - g_ref|| / ||g_ref|| over the tensors carrying >= 1e-6 of the squared gradient norm
                   (``grad_report``'s rule; sub-sampled entries for the large tensors),
  cosine           of the whole gradient with the golden over the sub-sampled entries, and of each trunk's gradient alone
                   (mlp_mean / mlp_weights: the mean trunk's 1 / sigma^2 dominates the whole, and the norm filter above leaves
                   small tensors of the weights trunk out -- the per-trunk cosine covers every tensor of it).
Each error bound is 2x the worst recorded value of its quantity over the family's cases; the cosine bound is the worst recorded
value minus half its distance to 1.
"""
import ctypes as C
import fnmatch
import os
import textwrap

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import get_class, instantiate, load_config
from oracle import dppo_oracle as O
from tests.golden.make_golden_bc_cases import (BC_CLAMPED, BC_GAUSS_CASES, BC_GMM_CASES, BC_GMM_NETS, BC_WEIGHT_SEED, clamp_mask,
                                               gauss_logvar, gmm_logvar)
from tests.golden.make_golden_cases import GAUSS_CASES

T = torch.from_numpy
SHIPPED_BC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_bc_cfgs.json")

# measured on the MI355X (profiles/bc_gaussian_parity.json, "worst/<family>/bf16"): 2 x the worst loss / gradient error of the
# family's cases, worst cosine - (1 - worst cosine) / 2 (whole gradient: cos; worst single trunk: cos_trunk).  The Gaussian
# head's entropy is a function of logvar alone (no bf16 operand reaches it), so it keeps the fp32 bound; the mixture's depends
# on softmax(logits) of a bf16 trunk: 2 x its worst.
BF16_BOUNDS = {
    "gaussian": dict(loss=2 * 1.4456e-4, entropy=None, grad=2 * 0.05110, cos=0.9999914 - 0.5 * (1 - 0.9999914),
                     cos_trunk=0.9999371 - 0.5 * (1 - 0.9999371)),
    "gmm": dict(loss=2 * 1.6351e-3, entropy=2 * 2.7591e-5, grad=2 * 0.07806, cos=0.9993910 - 0.5 * (1 - 0.9993910),
                cos_trunk=0.9987694 - 0.5 * (1 - 0.9987694)),
}


def shipped_bc(pattern):
    """(path, cfg) of every Gaussian / mixture pre-training cfg the reference ships whose path under cfg/ matches `pattern`
    (tests/golden/shipped_bc_cfgs.json, written by make_bc_cfg_fixture.py: resolved with device=cpu)."""
    cfgs = load_config(SHIPPED_BC)
    return [(p, cfgs[p]) for p in sorted(cfgs) if fnmatch.fnmatch(p, pattern)]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_every_shipped_gaussian_and_gmm_pretraining_cfg_resolves():
    """pre_gaussian_mlp.yaml with a fixed-std residual trunk (13) and pre_gmm_mlp.yaml (7): the agent target is
    TrainGaussianAgent, the model GaussianModel / GMMModel, the network builds and the C ABI counts the same parameters; the
    gym cfgs (plain trunk or state-dependent std) still refuse to build."""
    from dppo_amd import hip
    from dppo_amd.agent.pretrain.train_gaussian_agent import TrainGaussianAgent
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.gmm import GMMModel
    lib = hip.load()
    n_gauss = n_refused = 0
    for p, cfg in shipped_bc("*/pretrain/*/pre_gaussian_mlp.yaml"):
        assert get_class(cfg._target_) is TrainGaussianAgent, p
        assert get_class(cfg.model._target_) is GaussianModel, p
        node = cfg.model.network
        if node.get("fixed_std", None) is None or not node.get("residual_style", False):
            with pytest.raises(NotImplementedError):
                instantiate(node)
            n_refused += 1
            continue
        net = instantiate(node)
        assert lib.dppo_net_param_count(C.byref(net.net_desc())) == net.flat_params().numel(), (p, lib.dppo_last_error())
        assert net.flat_params().numel() == sum(q.numel() for q in net.mlp_mean.parameters()), p
        assert lib.dppo_gaussian_bc_workspace_bytes(C.byref(net.net_desc()), hip.PREC_BF16, int(cfg.train.batch_size)) > 0, p
        n_gauss += 1
    assert n_gauss == 13 and n_refused == 6
    n_gmm = 0
    for p, cfg in shipped_bc("*/pretrain/*/pre_gmm_mlp.yaml"):
        assert get_class(cfg._target_) is TrainGaussianAgent, p
        assert get_class(cfg.model._target_) is GMMModel, p
        net = instantiate(cfg.model.network)
        assert float(net.fixed_std) == pytest.approx(0.1) and not net.learn_fixed_std, p
        for t in (net.mean_net, net.weights_net):
            assert lib.dppo_net_param_count(C.byref(t.net_desc())) == t.flat_params().numel(), (p, lib.dppo_last_error())
        assert net.flat_params().numel() == net.mean_net.flat_params().numel() + net.weights_net.flat_params().numel()
        assert net.mean_net.net_desc().out_dim == int(cfg.action_dim) * int(cfg.horizon_steps) * int(cfg.num_modes)
        assert lib.dppo_gmm_bc_workspace_bytes(C.byref(net.mean_net.net_desc()), C.byref(net.weights_net.net_desc()), hip.PREC_BF16,
                                               int(cfg.train.batch_size)) > 0, p
        n_gmm += 1
    assert n_gmm == 7


def _cpu_gauss(learn):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    net = Gaussian_MLP(action_dim=2, horizon_steps=4, cond_dim=4, mlp_dims=[256, 256, 256], activation_type="ReLU",
                       residual_style=True, fixed_std=0.1, learn_fixed_std=learn, precision="fp32")
    return net, net.net_desc(), net.gaussian_cfg()


def test_gaussian_bc_entry_rejects_bad_arguments_on_the_host():
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch: every refusal below comes before the first launch
    err = lambda: lib.dppo_last_error().decode()
    net, d, cfg = _cpu_gauss(False)
    N = 64
    ws = lib.dppo_gaussian_bc_workspace_bytes(C.byref(d), hip.PREC_F32, N)
    assert ws > lib.dppo_gaussian_workspace_bytes(C.byref(d), None, hip.PREC_F32, N) > 0  # training buffers, not inference only
    assert lib.dppo_gaussian_bc_workspace_bytes(C.byref(d), hip.PREC_F32, 0) == -1 and "N out of range" in err()
    call = lambda cfg_, N_, params=X, lv=None, lvg=None, wsb=ws, out=X: lib.dppo_gaussian_bc_loss_fwd_bwd(
        C.byref(d), hip.PREC_F32, params, X, C.byref(cfg_), lv, X, X, N_, 0.0, X, lvg, out, X, wsb, None)
    assert call(cfg, N, params=None) == -1 and "null pointer" in err()
    assert call(cfg, N, out=None) == -1 and "null pointer" in err()
    assert call(cfg, 0) == -1 and "N out of range" in err()
    assert call(cfg, N, wsb=ws - 256) == -1 and "workspace too small" in err()
    _, _, cfg1 = _cpu_gauss(True)
    assert call(cfg1, N, lv=None) == -1 and "needs logvar" in err()
    assert call(cfg1, N, lv=X, lvg=None) == -1 and "needs logvar_grad" in err()
    bad = _cpu_gauss(False)[2]
    bad.action_dim = 3
    assert call(bad, N) == -1 and "out_dim" in err()
    # a learned std keeps 16 x Ta*Da logvar terms of a block in shared memory: refused with a message, not at the launch
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    wide = Gaussian_MLP(action_dim=100, horizon_steps=8, cond_dim=4, mlp_dims=[256, 256, 256], residual_style=True, fixed_std=0.1,
                        learn_fixed_std=True, precision="fp32")
    dw, cw = wide.net_desc(), wide.gaussian_cfg()
    wsw = lib.dppo_gaussian_bc_workspace_bytes(C.byref(dw), hip.PREC_F32, N)
    assert wsw > 0 and lib.dppo_gaussian_bc_loss_fwd_bwd(C.byref(dw), hip.PREC_F32, X, X, C.byref(cw), X, X, X, N, 0.0, X, X, X, X, wsw,
                                                         None) == -1 and "above 768" in err()


def test_gmm_bc_entry_rejects_bad_arguments_on_the_host():
    from dppo_amd import hip
    from dppo_amd.model.common.mlp_gmm import GMM_MLP
    lib = hip.load()
    X = 4096
    err = lambda: lib.dppo_last_error().decode()
    mk = lambda learn: GMM_MLP(action_dim=2, horizon_steps=4, cond_dim=4, mlp_dims=[256, 256], num_modes=5, activation_type="ReLU",
                               residual_style=False, fixed_std=0.1, learn_fixed_std=learn, precision="fp32")
    net = mk(False)
    m, w = net._trunks(bind=False)
    dm, dw = m.net_desc(), w.net_desc()
    N = 64
    ws = lib.dppo_gmm_bc_workspace_bytes(C.byref(dm), C.byref(dw), hip.PREC_F32, N)
    assert ws > lib.dppo_gmm_workspace_bytes(C.byref(dm), C.byref(dw), None, hip.PREC_F32, N) > 0
    assert lib.dppo_gmm_bc_workspace_bytes(C.byref(dm), C.byref(dw), hip.PREC_F32, 0) == -1 and "N out of range" in err()
    call = lambda cfg_, N_, wp=X, lv=None, lvg=None, wsb=ws, wg=X: lib.dppo_gmm_bc_loss_fwd_bwd(
        C.byref(dm), C.byref(dw), hip.PREC_F32, X, X, wp, X, C.byref(cfg_), lv, X, X, N_, X, wg, lvg, X, X, wsb, None)
    cfg = net.gmm_cfg()
    assert call(cfg, N, wp=None) == -1 and "null pointer" in err()
    assert call(cfg, N, wg=None) == -1 and "null pointer" in err()
    assert call(cfg, 0) == -1 and "N out of range" in err()
    assert call(cfg, N, wsb=ws - 256) == -1 and "workspace too small" in err()
    cfg1 = mk(True).gmm_cfg()
    assert call(cfg1, N, lv=None) == -1 and "needs logvar" in err()
    assert call(cfg1, N, lv=X, lvg=None) == -1 and "needs logvar_grad" in err()
    bad = net.gmm_cfg()
    bad.num_modes = 4
    assert call(bad, N) == -1 and "num_modes" in err()


# ---------------------------------------------------------------------------------------------------------------- GPU
def gauss_model(case, prec):
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    sname, kw = GAUSS_CASES[case]
    a, _ = O.named_specs(sname)
    actor = Gaussian_MLP(action_dim=a.action_dim, horizon_steps=a.horizon_steps, cond_dim=a.cond_dim, mlp_dims=list(a.mlp_dims),
                         activation_type=a.activation, residual_style=True, fixed_std=kw["fixed_std"],
                         learn_fixed_std=kw["learn_fixed_std"], std_min=kw["std_min"], std_max=kw["std_max"], precision=prec)
    sd = dict(O.init_params(a, BC_WEIGHT_SEED))
    lv = gauss_logvar(case, a.action_dim, kw)
    if lv is not None:
        sd["logvar"] = T(lv)
    actor.load_state_dict(sd, strict=False)
    return GaussianModel(network=actor, horizon_steps=a.horizon_steps, device="cuda:0")


def gmm_model(net_name, prec):
    from dppo_amd.model.common.gmm import GMMModel
    from dppo_amd.model.common.mlp_gmm import GMM_MLP
    cond, tkw, Ta, Da, gkw = BC_GMM_NETS[net_name]
    M = gkw["num_modes"]
    ms, ws = O.gmm_specs(cond, tkw["mlp_dims"], tkw["activation"], tkw["residual"], Da, Ta, M)
    actor = GMM_MLP(action_dim=Da, horizon_steps=Ta, cond_dim=cond, mlp_dims=list(tkw["mlp_dims"]), num_modes=M,
                    activation_type=tkw["activation"], residual_style=tkw["residual"], fixed_std=gkw["fixed_std"],
                    learn_fixed_std=gkw["learn_fixed_std"], std_min=gkw["std_min"], std_max=gkw["std_max"], precision=prec)
    sd = dict(O.gmm_init_params(ms, ws, BC_WEIGHT_SEED))
    sd["logvar_min"], sd["logvar_max"] = actor.logvar_min.data.clone(), actor.logvar_max.data.clone()
    lv = gmm_logvar(net_name, Da, gkw)
    if lv is not None:
        sd["logvar"] = T(lv)
    actor.load_state_dict(sd, strict=True)
    return GMMModel(network=actor, horizon_steps=Ta, device="cuda:0")


def family_setup(family, case, prec, golden):
    """(model, fixture, key prefix, ent_coef) of one case: `case` is a BC_GAUSS_CASES name or a BC_GMM_CASES (net, kind) pair."""
    if family == "gaussian":
        return gauss_model(case, prec), golden("g22_gaussian_bc"), case, BC_GAUSS_CASES[case]
    return gmm_model(case[0], prec), golden("g23_gmm_bc"), f"{case[0]}_{case[1]}", None


def clamped_entries(family, case):
    """Boolean mask of the logvar entries OUTSIDE the clamp range (None for a fixed std): all False except in the BC_CLAMPED
    cases, which must have some -- the clamp's pass-through in the loss and in the entropy bonus is exercised with zeros."""
    if family == "gaussian":
        kw = GAUSS_CASES[case][1]
        lv = gauss_logvar(case, O.named_specs(GAUSS_CASES[case][0])[0].action_dim, kw)
        name = case
    else:
        _, _, _, Da, kw = BC_GMM_NETS[case[0]]
        lv = gmm_logvar(case[0], Da, kw)
        name = case[0]
    if lv is None:
        return None
    out = ~clamp_mask(lv, kw)
    assert out.any() == (name in BC_CLAMPED)
    return out


def run_loss(model, state, action, ent_coef):
    """One ``loss`` call + backward -> (loss, entropy, [(name, grad)] over the network's parameters, raw flat results)."""
    for p in model.network.parameters():
        p.grad = None
    cond = {"state": state}
    loss, info = model.loss(action, cond, ent_coef) if ent_coef is not None else model.loss(action, cond)
    raw = (loss.detach().clone(), info["entropy"].clone(), model.last_loss_grad.clone(),
           None if model.last_logvar_grad is None else model.last_logvar_grad.clone())
    loss.backward()
    named = [(k, p.grad) for k, p in model.network.named_parameters() if p.grad is not None]
    return float(raw[0]), float(raw[1]), named, raw


def bf16_errors(g, prefix, named, loss, entropy):
    """The three measured quantities of the module docstring (+ the entropy's error, same definition as the loss's)."""
    ref_l, ref_e = float(g[f"{prefix}_loss"]), float(g[f"{prefix}_entropy"])
    per, n_ref, num, a2, b2, trunk = [], 0.0, 0.0, 0.0, 0.0, {}
    for k, grad in named:
        x = grad.double().cpu().numpy().reshape(-1)
        key = f"{prefix}_g_{k}"
        if key in g:
            r, xs = g[key].astype(np.float64).reshape(-1), x
            nr = float(r @ r)
        else:
            r, xs, nr = g[key + "__sub"].astype(np.float64), x[::61], float(g[key + "__norm"]) ** 2
        per.append((k, nr, float(np.linalg.norm(xs - r) / (np.linalg.norm(r) + 1e-30))))
        n_ref += nr
        num, a2, b2 = num + float(xs @ r), a2 + float(xs @ xs), b2 + float(r @ r)
        if k != "logvar":  # per trunk (mlp_mean / mlp_weights): the mean trunk's 1 / sigma^2 would hide the weights trunk
            t = trunk.setdefault(k.split(".")[0], [0.0, 0.0, 0.0])
            t[0], t[1], t[2] = t[0] + float(xs @ r), t[1] + float(xs @ xs), t[2] + float(r @ r)
    cos_trunk = {k: t[0] / np.sqrt(t[1] * t[2]) for k, t in trunk.items()}
    worst = max((e, k) for k, nr, e in per if nr >= 1e-6 * n_ref)
    return dict(loss=abs(loss - ref_l) / max(1.0, abs(ref_l)), entropy=abs(entropy - ref_e) / max(1.0, abs(ref_e)),
                grad=worst[0], grad_tensor=worst[1], cos=num / np.sqrt(a2 * b2), cos_trunk=min(cos_trunk.values()), cos_trunks=cos_trunk,
                per_tensor={k: e for k, _, e in per})


ALL_CASES = [("gaussian", c) for c in sorted(BC_GAUSS_CASES)] + [("gmm", c) for c in BC_GMM_CASES]
case_id = lambda fc: fc[1] if fc[0] == "gaussian" else f"{fc[1][0]}_{fc[1][1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("fc", ALL_CASES, ids=case_id)
def test_hip_bc_loss_entropy_and_every_gradient(golden, fc, prec):
    """GaussianModel.loss / GMMModel.loss against the reference's loss, entropy and loss.backward() on every case of g22 / g23
    (the mixture's *far* cases included: the loss must be finite where a naive exp underflows every mode).  fp32: the bounds
    tests/test_gaussian.py:128 / tests/test_gmm.py:102-106 hold these trunks to, and bit-stable from call to call."""
    from tests.test_unet import grad_report
    family, case = fc
    model, g, prefix, ent_coef = family_setup(family, case, prec, golden)
    state, action = T(g[f"{prefix}_state"]).cuda(), T(g[f"{prefix}_true_action"]).cuda()
    loss, entropy, named, raw = run_loss(model, state, action, ent_coef)
    ref_l, ref_e = float(g[f"{prefix}_loss"]), float(g[f"{prefix}_entropy"])
    print(f"{prefix} {prec}: loss {loss!r} ref {ref_l!r} entropy {entropy!r} ref {ref_e!r}")
    assert np.isfinite(loss) and np.isfinite(entropy) and all(bool(torch.isfinite(x).all()) for _, x in named)
    want = {k[len(prefix) + 3:].split("__")[0] for k in g if k.startswith(prefix + "_g_")}
    assert {k for k, _ in named} == want  # both trunks and logvar (when learned): every gradient the reference has
    out = clamped_entries(family, case)
    if out is not None and out.any():
        # a clamped logvar entry gets NO gradient, from the likelihood or from the entropy bonus (the reference's is exactly 0
        # there; grad_report's norm filter would not see an error on a zero reference)
        glv = dict(named)["logvar"].cpu().numpy()
        assert not g[f"{prefix}_g_logvar"][out].any() and not glv[out].any(), (glv, out)
        assert family == "gaussian" or glv[~out].all()  # ... and the mixture case has passing entries beside them
    if prec == "fp32":
        rtol, atol = (2e-4, 2e-5) if family == "gaussian" else (2e-3, 2e-4)
        (worst, e), nerr = grad_report(g, f"{prefix}_g", named)
        print(f"  gradients: worst tensor {worst} {e:.3e}, norm error {nerr:.3e}")
        assert abs(loss - ref_l) <= rtol * abs(ref_l) + atol * max(1.0, abs(ref_l)), (loss, ref_l)
        assert abs(entropy - ref_e) <= rtol * abs(ref_e) + atol * max(1.0, abs(ref_e)), (entropy, ref_e)
        assert e < 1e-2 and nerr < 2e-3, (worst, e, nerr)
        again = run_loss(model, state, action, ent_coef)[3]
        for x, y in zip(raw, again):
            assert (x is None and y is None) or torch.equal(x, y)
    else:
        m, b = bf16_errors(g, prefix, named, loss, entropy), BF16_BOUNDS[family]
        print(f"  bf16: loss error {m['loss']:.3e} entropy error {m['entropy']:.3e} gradient error {m['grad']:.3e} "
              f"({m['grad_tensor']}) cosine {m['cos']:.6f} per trunk {m['cos_trunks']}")
        assert m["loss"] <= b["loss"], (m, b)
        if b["entropy"] is None:
            assert abs(entropy - ref_e) <= 2e-4 * abs(ref_e) + 2e-5 * max(1.0, abs(ref_e)), (entropy, ref_e)
        else:
            assert m["entropy"] <= b["entropy"], (m, b)
        assert m["grad"] <= b["grad"] and m["cos"] >= b["cos"] and m["cos_trunk"] >= b["cos_trunk"], (m, b)


@pytest.mark.gpu
@pytest.mark.parametrize("fc", ALL_CASES, ids=case_id)
def test_hip_bc_gradients_of_two_half_batches_add_up(golden, fc):
    """The gradient (logvar's included) and the loss of one N = 64 call equal the mean of two N = 32 calls on the halves within
    the fp32 bounds above: catches a wrong 1 / B or 1 / (B Ta Da) and partial sums that depend on the launch geometry."""
    family, case = fc
    model, g, prefix, ent_coef = family_setup(family, case, "fp32", golden)
    state, action = T(g[f"{prefix}_state"]).cuda(), T(g[f"{prefix}_true_action"]).cuda()
    l64, e64, whole, _ = run_loss(model, state, action, ent_coef)
    halves = [run_loss(model, state[lo:lo + 32].contiguous(), action[lo:lo + 32].contiguous(), ent_coef) for lo in (0, 32)]
    lh, eh = 0.5 * (halves[0][0] + halves[1][0]), 0.5 * (halves[0][1] + halves[1][1])
    rtol, atol = (2e-4, 2e-5) if family == "gaussian" else (2e-3, 2e-4)
    assert abs(lh - l64) <= rtol * abs(l64) + atol * max(1.0, abs(l64)) and abs(eh - e64) <= rtol * abs(e64) + atol * max(1.0, abs(e64))
    n_got = n_ref = 0.0
    per = []
    for (k, gw), (ka, ga), (kb, gb) in zip(whole, halves[0][2], halves[1][2]):
        assert k == ka == kb
        ref, got = gw.double(), 0.5 * (ga.double() + gb.double())
        per.append((k, float(ref.norm()) ** 2, float((got - ref).norm() / (ref.norm() + 1e-30))))
        n_got, n_ref = n_got + float(got.norm()) ** 2, n_ref + float(ref.norm()) ** 2
    worst = max((e, k) for k, nr, e in per if nr >= 1e-6 * n_ref)
    print(f"{prefix}: worst tensor {worst[1]} {worst[0]:.3e}, norm error {abs(np.sqrt(n_got / n_ref) - 1.0):.3e}")
    assert worst[0] < 1e-2 and abs(np.sqrt(n_got / n_ref) - 1.0) < 2e-3, (worst, n_got, n_ref)


HEAD = textwrap.dedent("""
    _target_: dppo.agent.pretrain.train_gaussian_agent.TrainGaussianAgent
    logdir: ${oc.env:DPPO_LOG_DIR}/pretrain
    seed: 42
    device: cuda:0
    obs_dim: 11
    action_dim: 3
    horizon_steps: 4
    cond_steps: 1
    num_modes: 5
    wandb: null
    train:
      n_epochs: 6
      batch_size: 128
      learning_rate: 1e-3
      weight_decay: 1e-6
      lr_scheduler: {first_cycle_steps: 200, warmup_steps: 1, min_lr: 1e-4}
      save_model_freq: 100
      epoch_start_ema: 2
      update_ema_freq: 2
      ent_coef: 0.01
    ema:
      decay: 0.9
""")
YAML_GAUSS = HEAD + textwrap.dedent("""
    model:
      _target_: dppo.model.common.gaussian.GaussianModel
      network:
        _target_: dppo.model.common.mlp_gaussian.Gaussian_MLP
        mlp_dims: [256, 256, 256]
        activation_type: ReLU
        residual_style: True
        fixed_std: 0.1
        learn_fixed_std: True
        std_min: 0.01
        std_max: 0.2
        cond_dim: ${eval:'${obs_dim} * ${cond_steps}'}
        horizon_steps: ${horizon_steps}
        action_dim: ${action_dim}
      horizon_steps: ${horizon_steps}
      device: ${device}
""")
YAML_GMM = HEAD + textwrap.dedent("""
    model:
      _target_: dppo.model.common.gmm.GMMModel
      network:
        _target_: dppo.model.common.mlp_gmm.GMM_MLP
        mlp_dims: [512, 512, 512]
        residual_style: True
        fixed_std: 0.1
        num_modes: ${num_modes}
        cond_dim: ${eval:'${obs_dim} * ${cond_steps}'}
        horizon_steps: ${horizon_steps}
        action_dim: ${action_dim}
      horizon_steps: ${horizon_steps}
      device: ${device}
""")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gaussian", "gmm"])
def test_gaussian_pretraining_runs_and_its_checkpoint_feeds_fine_tuning(tmp_path, monkeypatch, family):
    from dppo_amd.agent.dataset.sequence import synthetic_dataset
    from dppo_amd.model.common.critic import CriticObs
    monkeypatch.setenv("DPPO_LOG_DIR", str(tmp_path))
    p = tmp_path / "pre.yaml"
    p.write_text(YAML_GAUSS if family == "gaussian" else YAML_GMM)
    cfg = load_config(str(p))
    ds = synthetic_dataset(11, 3, 4, cond_steps=1, n_traj=24, traj_len=48, seed=1, device="cuda:0")
    agent = get_class(cfg._target_)(cfg, dataset=ds)
    assert type(agent).__name__ == "TrainGaussianAgent" and agent.ent_coef == pytest.approx(0.01)
    w0 = agent.net.flat_params().clone()
    hist = agent.run()
    print([(h["loss"], h["entropy"]) for h in hist])
    assert len(hist) == 6 and all(set(h) == {"epoch", "loss", "entropy"} for h in hist)
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["entropy"]) for h in hist)
    assert hist[-1]["loss"] < hist[0]["loss"], hist  # NLL dominated by (a - mu)^2 / 2 sigma^2 at sigma 0.1: any working update lowers it
    assert not torch.equal(agent.net.flat_params(), w0)
    assert not torch.equal(agent.ema_flat, agent.net.flat_params())  # the EMA lags the model
    ck = os.path.join(str(tmp_path), "pretrain", "checkpoint", "state_6.pt")
    data = torch.load(ck, weights_only=True)
    assert data["epoch"] == 6 and set(data) == {"epoch", "model", "ema"}
    for part in ("model", "ema"):
        assert "network.mlp_mean.layers.1.l1.weight" in data[part] and "network.logvar_min" in data[part]
        assert ("network.logvar" in data[part]) == (family == "gaussian")
        assert ("network.mlp_weights.layers.1.l1.weight" in data[part]) == (family == "gmm")
    critic = CriticObs(cond_dim=11, mlp_dims=[256, 256, 256], residual_style=True)
    if family == "gaussian":
        from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
        from dppo_amd.model.rl.gaussian_ppo import PPO_Gaussian
        assert not torch.equal(agent.ema_logvar, agent.net.logvar.data)
        assert torch.equal(data["ema"]["network.logvar"].cuda(), agent.ema_logvar)
        actor = Gaussian_MLP(action_dim=3, horizon_steps=4, cond_dim=11, mlp_dims=[256, 256, 256], activation_type="ReLU",
                             residual_style=True, fixed_std=0.1, learn_fixed_std=True, std_min=0.01, std_max=0.2)
        ft = PPO_Gaussian(actor=actor, critic=critic, horizon_steps=4, device="cuda:0", clip_ploss_coef=0.01, network_path=ck)
        assert torch.equal(ft.actor_ft.logvar.data, agent.net.logvar.data) and torch.equal(ft.actor.logvar.data, agent.net.logvar.data)
        assert torch.equal(ft.actor.flat_params(), agent.net.flat_params())
    else:
        from dppo_amd.model.common.mlp_gmm import GMM_MLP
        from dppo_amd.model.rl.gmm_ppo import PPO_GMM
        actor = GMM_MLP(action_dim=3, horizon_steps=4, cond_dim=11, mlp_dims=[512, 512, 512], num_modes=5, residual_style=True,
                        fixed_std=0.1)
        ft = PPO_GMM(actor=actor, critic=critic, horizon_steps=4, device="cuda:0", clip_ploss_coef=0.01, network_path=ck)
    # these two load checkpoint["model"], not ["ema"] (model/common/gaussian.py, gmm.py, as the reference does)
    assert torch.equal(ft.actor_ft.flat_params(), agent.net.flat_params())
    assert not torch.equal(ft.actor_ft.flat_params(), agent.ema_flat)
    a = ft(cond={"state": ds.states[:8, None]}, deterministic=True)
    assert tuple(a.shape) == (8, 4, 3) and torch.isfinite(a).all()
    # the plain model classes load it too
    reloaded = instantiate(dict(cfg.model, network_path=ck))
    assert torch.equal(reloaded.network.flat_params(), agent.net.flat_params())
