"""SAC fine-tuning (reference model/rl/gaussian_sac.py, model/common/gaussian.py:85-120, model/common/mlp_gaussian.py:304-379,
agent/finetune/train_sac_agent.py): the shipped SAC cfg resolves, ``SAC_Gaussian`` carries the reference's state dict, the new C ABI
entries check their arguments, and the plain-torch restatement of tests/golden/make_golden_sac_cases.py reproduces the g27 fixture
the reference wrote (CPU).  On the GPU the sample, the three losses and every gradient are held to the restatement in FLOAT64 fed
the same fp32 values -- for the actor loss evaluated on the call's own ``sel`` (which trunk is the smaller, per row), which the
inputs' guard band makes the fixture's.  ReLU's derivative has an edge at 0: check_on_own_sel hands the few gates within
make_golden_dql_cases.RELU_TIE of it over, as tests/test_dql.py does.

Saturation.  In the ``tiny_sat`` case |u| reaches 12, where the reference's own fp32 ``1 - tanh(u)^2`` cancels: no tolerance is fixed
for its sample.  e_ref is the error of the reference's fp32 g27 value against the float64 restatement (max over the case); the call
may be off from float64 by at most 2 e_ref.

bf16.  No tolerance is fixed: the yardstick is the restatement with every Linear's operands rounded to bf16
(make_golden_dql_cases.bf16_linears) on the call's own ``sel``; with e_y its error against the fp32 restatement on the same ``sel``,
the call may be off by at most 2 e_y (loss, d_a, per tensor, 1 - cosine).  tools/sac_parity_report.py writes the measured figures to
profiles/sac_parity.json; nothing here reads that file.
"""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import Cfg, get_class, instantiate, load_config
from tests.golden import make_golden_sac_cases as K
from tests.test_dql import check_stepped, grad_violations, rel_errors, stats_close
from tests.test_idql import check_grads_fp32
from tests.test_qsm import close_to_fixture, ring_of

T = torch.from_numpy
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_sac_cfgs.json")
SAC_CFG = "gym/scratch/halfcheetah-v2/sac_mlp.yaml"
IDS = [f"{c}_{n}" for c, n in K.CASES]
PLAIN = [(c, n) for c, n in K.CASES if (c, n) not in K.SAT_CASES]
PLAIN_IDS = [f"{c}_{n}" for c, n in PLAIN]
D64 = torch.float64


def make_actor(case, prec="fp32"):
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    od, ta, da = K.shapes(case)
    net = Gaussian_MLP(da, ta, od, mlp_dims=K.dims(case), activation_type=K.activation(case), tanh_output=False, fixed_std=None,
                       std_min=K.STD_MIN, std_max=K.STD_MAX, precision=prec)
    net.load_state_dict(K.actor_params(case), strict=True)
    return net


def make_q(case, prec="fp32", **kw):
    from dppo_amd.model.common.critic import CriticObsAct
    od, ta, da = K.shapes(case)
    return CriticObsAct(**dict(dict(cond_dim=od, mlp_dims=K.dims(case), action_dim=da, action_steps=ta,
                                    activation_type=K.activation(case), precision=prec), **kw))


def make_model(case, prec, device, squash=True):
    from dppo_amd.model.rl.gaussian_sac import SAC_Gaussian
    q = make_q(case, prec)
    q.load_state_dict(K.twin_params(case), strict=True)
    m = SAC_Gaussian(actor=make_actor(case, prec), critic=q, horizon_steps=K.shapes(case)[1], device=device,
                     randn_clip_value=K.RANDN_CLIP, tanh_output=squash)
    m.target_critic.load_state_dict(K.twin_params(case, K.TARGET_EPS), strict=True)
    return m


def named(module, flat):
    """(state-dict name, slice of ``flat``) in the flat image's order (``trunk_parameters``: the two heads' weights, then biases)."""
    names = {id(p): k for k, p in module.named_parameters()}
    out, off = [], 0
    for p in module.trunk_parameters():
        out.append((names[id(p)], flat[off:off + p.numel()].view(p.shape)))
        off += p.numel()
    assert off == flat.numel()
    return out


def by_name(pairs, order):
    d = dict(pairs)
    return [(k, d[k]) for k in order]


@functools.lru_cache(maxsize=None)
def restated(case, n, dtype=D64):
    """The restatement of one case: computed once, shared, never modified."""
    b, a, q = K.inputs(case, n), K.leaf(K.actor_params(case), dtype), K.leaf(K.twin_params(case), dtype)
    with K.relu_gates() as rg:
        ra = K.loss_actor(a, K.twin_params(case), case, b, dtype=dtype)
    rc = K.loss_critic(q, K.twin_params(case, K.TARGET_EPS), K.actor_params(case), case, b, dtype=dtype)
    lt, gt, logp_t = K.loss_temperature(K.actor_params(case), case, b, K.SEQ_LOG_ALPHA, dtype=dtype)
    with torch.no_grad():
        det = K.sample(K.cast(K.actor_params(case), dtype), case, b["obs"].to(dtype), b["noise"], deterministic=True)
    ra["named"], rc["named"] = list(zip(K.grad_names(a), ra["grads"])), list(zip(q, rc["grads"]))
    return dict(actor=ra, critic=rc, t=(float(lt), float(gt), logp_t), det=det, near_zero=rg.near_zero(), calls=rg.calls)


def restate_actor_on(case, n, sel, bf16=False, gates=None, dtype=D64, squash=True):
    a = K.leaf(K.actor_params(case), dtype)
    with gates if gates is not None else K.relu_gates() as rg:
        if bf16:
            with K.bf16_linears():
                res = K.loss_actor(a, K.twin_params(case), case, K.inputs(case, n), dtype=dtype, sel=sel, squash=squash)
        else:
            res = K.loss_actor(a, K.twin_params(case), case, K.inputs(case, n), dtype=dtype, sel=sel, squash=squash)
    res["named"], res["near_zero"] = list(zip(K.grad_names(a), res["grads"])), rg.near_zero()
    return res


def check_on_own_sel(case, n, sel, got_named, d_a, what):
    """d_a and every gradient of a run against the float64 restatement on the run's ``sel``, by grad_violations' rule on EVERY
    entry.  Where that misses and the networks are ReLU ones, the yardstick's gates below RELU_TIE are tried on their other side,
    nearest to zero first, each kept if it lowers the count of entries outside the rule (tests/test_dql.py::check_on_own_chain)."""
    ref = restate_actor_on(case, n, sel)
    order = [k for k, _ in ref["named"]]
    got = [("d_a", d_a)] + by_name(got_named, order)
    bad = grad_violations([("d_a", ref["d_a"])] + ref["named"], got)
    if not bad or K.activation(case) != "ReLU":
        assert not bad, (what, bad)
        return
    count = lambda b: sum(x[1] + int(x[3]) for x in b)
    print(f"{what}: {count(bad)} entries outside the rule {bad}; {len(ref['near_zero'])} ReLU gates below {K.RELU_TIE:g}")
    force = {}
    for z, where, gate in ref["near_zero"]:
        trial = dict(force)
        trial[where] = not gate
        res = restate_actor_on(case, n, sel, gates=K.relu_gates(trial))
        now = grad_violations([("d_a", res["d_a"])] + res["named"], got)
        if count(now) < count(bad):
            force, bad = trial, now
        if not bad:
            return
    assert not bad, (what, bad, force)


def check_stepped_twice(g, key, named_w, gkeys, lr):
    """check_stepped's rule for weights that took TWO Adam steps (the sequence's actor).  The first step is lr g0 / (|g0| + eps): an
    entry whose gradient is off by dg0 (the gradient rule: rtol 2e-3, the tensor's atol) moves off by lr dg0 / |g0|, at most 2 lr.
    The second is lr m / (sqrt(v) + eps) with m = 0.474 g0 + 0.526 g1 and v = 0.4997 g0^2 + 0.5003 g1^2 after bias correction:
    sqrt(v) >= 0.707 max(|g0|, |g1|), and its derivative by either gradient is below 1.5 / max(|g0|, |g1|), so it moves off by
    at most 1.5 lr (dg0 + dg1) / max(|g0|, |g1|), at most 2 lr.  Plus one ulp-class term for the weight; nearly all entries tight."""
    for k, p in named_w:
        x = p.detach().cpu().numpy()
        full = f"{key}_{k}" in g
        ref = g[f"{key}_{k}"] if full else g[f"{key}_{k}__sub"]
        xs = x if full else x.reshape(-1)[::61]
        gs, atols = [], []
        for gk in gkeys:
            gr = g[f"{gk}_{k}"] if full else g[f"{gk}_{k}__sub"]
            gn = float(np.linalg.norm(gr)) if full else float(g[f"{gk}_{k}__norm"])
            gs.append(np.abs(gr).astype(np.float64))
            atols.append(2e-4 * max(gn, 1e-8) / np.sqrt(x.size) + 1e-7)
        dg = [2e-3 * a + t for a, t in zip(gs, atols)]
        first = np.minimum(2.0, dg[0] / (gs[0] + 1e-8))
        second = np.minimum(2.0, 1.5 * (dg[0] + dg[1]) / (np.maximum(gs[0], gs[1]) + 1e-8))
        tol = lr * (first + second) + 1e-6 * np.abs(ref) + 1e-7
        assert (np.abs(xs - ref) <= tol).all(), (key, k, float(np.abs(xs - ref).max()))
        assert (np.abs(xs - ref) <= 2 * lr * 1e-2 + 1e-6 * np.abs(ref) + 1e-7).mean() > 0.99, (key, k)


def rel_close(got, ref, tol, what, per_row=False):
    """|got - ref| <= tol |ref|, entry by entry: a relative bound.  ``per_row``: ``ref`` holds one log-probability per row, a sum of
    O(1) terms of both signs that comes as near to 0 as 3e-3 in these cases; no fp32 evaluation can keep such an entry to 1e-5 of
    ITSELF, so the bound is ``tol`` times the array's largest |ref| (close_to_fixture's rule for tensors)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / (np.abs(ref).max() if per_row else np.abs(ref))
    print(f"{what}: {got} ref {ref} err {err.max():.2e}")
    assert err.max() <= tol, (what, got, ref)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_shipped_sac_cfg_resolves():
    from dppo_amd import hip
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_sac import SAC_Gaussian
    lib = hip.load()
    cfgs = load_config(SHIPPED)
    assert list(cfgs) == [SAC_CFG]
    cfg = cfgs[SAC_CFG]
    assert get_class(cfg._target_) is TrainSACAgent
    assert get_class(cfg.model._target_) is SAC_Gaussian and get_class(cfg.model.critic._target_) is CriticObsAct
    assert cfg.model.tanh_output is True and cfg.model.actor.tanh_output is False and "fixed_std" not in cfg.model.actor
    m = instantiate(cfg.model)
    assert type(m) is SAC_Gaussian and type(m.network) is Gaussian_MLP and m.target_critic is not m.critic
    da, dq = m.network.net_desc(), m.critic.net_desc()
    od, af = cfg.obs_dim * cfg.cond_steps, cfg.action_dim * cfg.horizon_steps
    assert (da.kind, da.plain, da.in_dim, da.hidden, da.n_blocks, da.out_dim) == (1, 1, od, 256, 1, 2 * af)
    assert dq.plain == 1 and dq.in_dim == od + af
    assert lib.dppo_net_param_count(C.byref(da)) == m.network.flat_params().numel() == sum(p.numel() for p in m.network.trunk_parameters())
    N = int(cfg.train.batch_size)
    for prec in (hip.PREC_F32, hip.PREC_BF16):
        assert lib.dppo_sac_actor_workspace_bytes(C.byref(da), C.byref(dq), prec, od, N) > 0, lib.dppo_last_error()
        assert lib.dppo_sac_q_loss_workspace_bytes(C.byref(dq), prec, od, N) > 0
        assert lib.dppo_sac_sample_workspace_bytes(C.byref(da), prec, N) > 0


def test_sac_state_dict_is_the_references(golden):
    g = golden("g27_sac")
    sd = make_model("cheetah", "fp32", "cpu").state_dict()
    assert len(sd) == 34 and list(sd) == [str(k) for k in g["state_dict_keys"]]
    assert [",".join(str(int(x)) for x in v.shape) for v in sd.values()] == [str(s) for s in g["state_dict_shapes"]]
    assert {k.split(".")[0] for k in sd} == {"network", "critic", "target_critic"}
    assert list(sd)[:2] == ["network.logvar_min", "network.logvar_max"]


@pytest.mark.parametrize("case", ["cheetah", "tiny", "chunk"])
def test_flat_layout_is_the_plain_trunks_with_the_heads_stacked(case):
    from dppo_amd import hip
    net = make_actor(case)
    od, ta, da = K.shapes(case)
    af, H = ta * da, K.dims(case)[-1]
    d = net.net_desc()
    flat = net.flat_params()
    assert hip.load().dppo_net_param_count(C.byref(d)) == flat.numel()
    p = K.actor_params(case)
    tail = torch.cat([p["mlp_mean.moduleList.0.linear_1.weight"].reshape(-1), p["mlp_logvar.moduleList.0.linear_1.weight"].reshape(-1),
                      p["mlp_mean.moduleList.0.linear_1.bias"], p["mlp_logvar.moduleList.0.linear_1.bias"]])
    assert tail.numel() == 2 * af * H + 2 * af and torch.equal(flat[-tail.numel():], tail)  # W (2 AF x H), then b (2 AF)
    assert [k for k, _ in named(net, flat)][-4:] == ["mlp_mean.moduleList.0.linear_1.weight", "mlp_logvar.moduleList.0.linear_1.weight",
                                                    "mlp_mean.moduleList.0.linear_1.bias", "mlp_logvar.moduleList.0.linear_1.bias"]
    assert list(net.state_dict()) == list(p)  # the state dict keeps the reference's names and order


def test_what_raised_before_still_raises():
    from dppo_amd.model.common.gaussian import GaussianModel
    from dppo_amd.model.common.mlp_gaussian import Gaussian_MLP
    from dppo_amd.model.rl.gaussian_sac import SAC_Gaussian
    with pytest.raises(NotImplementedError):
        Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], fixed_std=None, tanh_output=True)
    with pytest.raises(NotImplementedError):
        Gaussian_MLP(3, 1, 11, mlp_dims=[256, 256, 256], fixed_std=None, tanh_output=False, residual_style=True)
    with pytest.raises(NotImplementedError):
        Gaussian_MLP(3, 1, 11, mlp_dims=[64, 64], fixed_std=0.1, residual_style=False)
    fixed = Gaussian_MLP(3, 1, 11, mlp_dims=[256, 256, 256], fixed_std=0.1, residual_style=True)
    with pytest.raises(NotImplementedError, match="SAMPLED"):
        GaussianModel(fixed, 1, device="cpu", tanh_output=True)
    gm = GaussianModel(fixed, 1, device="cpu")
    for kw in (dict(get_logprob=True), dict(reparameterize=True)):
        with pytest.raises(NotImplementedError, match="out of scope"):
            gm({"state": torch.zeros(2, 1, 11)}, **kw)
    with pytest.raises(NotImplementedError, match="state-dependent"):
        SAC_Gaussian(actor=fixed, critic=make_q("tiny"), horizon_steps=1, device="cpu", tanh_output=True)
    with pytest.raises(ValueError, match="twin critic"):
        SAC_Gaussian(actor=make_actor("tiny"), critic=make_q("tiny", double_q=False), horizon_steps=1, device="cpu", tanh_output=True)
    with pytest.raises(NotImplementedError):
        make_actor("tiny").gaussian_cfg()


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_inputs_keep_their_guard_bands(case, n):
    """On the float64 restatement fed the fp32 values: every |q1 - q2| and every ||z| - randn_clip| sits at least ten times that
    quantity's fp32 ceiling away from its edge; outside the ``sat`` case |u| <= 2; in it |u| reaches 10 and |z| crosses the clip."""
    r, b = restated(case, n), K.inputs(case, n)
    gap = (r["actor"]["q1"] - r["actor"]["q2"]).abs().min().item()
    assert gap >= 10 * K.Q_CEIL, gap
    for key in ("noise", "noise_next", "noise_t", "noise2", "noise_t2"):
        z = b[key].double().abs()
        assert (z - K.RANDN_CLIP).abs().min().item() >= 10 * K.Z_CEIL * K.RANDN_CLIP, key
    u = r["actor"]["u"].abs()
    if (case, n) in K.SAT_CASES:
        z = b["noise"].abs()
        assert u.max() >= 10 and u.min() <= 0.1 and (z > K.RANDN_CLIP).any() and (z < K.RANDN_CLIP).any()
    else:
        assert u.max() <= K.U_MAX, u.max()
    assert 0 < len(r["calls"]) if K.activation(case) == "ReLU" else True


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_restatement_reproduces_the_reference_fixture(golden, case, n):
    """The fp32 restatement against g27: values within 1e-5 relative (rel_close; samples by close_to_fixture's rule), ``sel``
    equal, gradients by check_grads_fp32's rule."""
    g, name, r = golden("g27_sac"), f"{case}_{n}", restated(case, n, torch.float32)
    ra, rc = r["actor"], r["critic"]
    close_to_fixture(g, f"{name}_a", ra["a"], name)
    close_to_fixture(g, f"{name}_a_det", r["det"]["a"], name)
    rel_close(ra["logp"].numpy(), g[f"{name}_logp"], 1e-5, f"{name} logp", per_row=True)
    rel_close(r["det"]["logp"].numpy(), g[f"{name}_logp_det"], 1e-5, f"{name} logp_det", per_row=True)
    rel_close(rc["stats"], g[f"{name}_c_stats"], 1e-5, f"{name} critic")
    rel_close(ra["stats"], g[f"{name}_a_stats"], 1e-5, f"{name} actor")
    rel_close(r["t"][:2], g[f"{name}_t"], 1e-5, f"{name} temperature")
    assert np.array_equal(ra["sel"].astype(np.uint8), g[f"{name}_sel"])
    check_grads_fp32(g, name, [("d_a", ra["d_a"])])
    check_grads_fp32(g, f"{name}_ga", ra["named"])
    check_grads_fp32(g, f"{name}_gq", rc["named"])


@pytest.mark.parametrize("case,n", [("cheetah", 77), ("chunk", 77), ("tiny_sat", 77)])
def test_analytic_head_gradient_is_autograds(case, n):
    """The head's backward as the kernels implement it (sac.h) against autograd on the float64 restatement."""
    b, p = K.inputs(case, n), K.leaf(K.actor_params(case), D64)
    q = K.cast(K.twin_params(case), D64)
    s = K.sample(p, case, b["obs"].double(), b["noise"])
    q1, q2 = K.twin_forward(q, case, b["obs"].double(), s["a"])
    qs = torch.min(q1, q2)
    loss = (-qs + K.ALPHA * s["logp"]).mean()
    g = torch.autograd.grad(qs.sum(), s["a"], retain_graph=True)[0]
    dmean, draw = torch.autograd.grad(loss, [s["mean"], s["raw"]])
    zc = b["noise"].double().reshape(n, -1).clamp(-K.RANDN_CLIP, K.RANDN_CLIP)
    du, dr = K.head_backward({k: v.detach() for k, v in s.items()}, g, zc, K.ALPHA, n, p["logvar_min"].detach(), p["logvar_max"].detach())
    for got, want in ((du, dmean), (dr, draw)):
        assert (got - want).abs().max() <= 1e-9 * want.abs().max() + 1e-15, ((got - want).abs().max(), want.abs().max())


def test_restatement_reproduces_the_recorded_sequence(golden):
    g = golden("g27_sac")
    seq = K.restate_sequence()
    close_to_fixture(g, "seq_c_loss", seq["c_loss"], "seq")
    rel_close(seq["a_loss"], g["seq_a_loss"], 1e-5, "seq actor")
    rel_close(seq["t_loss"], g["seq_t_loss"], 1e-5, "seq temperature")
    rel_close(seq["log_alpha"], g["seq_log_alpha"], 1e-6, "seq log_alpha")
    assert float(g["seq_a_loss"][0]) != float(g["cheetah_77_a_stats"][0])  # the stepped critic moved the actor's loss
    for k, v in seq["gq"].items():
        close_to_fixture(g, f"seq_gq_{k}", v, "seq")
    for i in (0, 1):
        check_grads_fp32(g, f"seq_ga{i}", list(seq["ga"][i].items()))
    for key, gkey, step in (("q", "seq_gq", K.SEQ_LR), ("target", "seq_gq", K.SEQ_LR * K.SEQ_TAU)):
        check_stepped(g, f"seq_{key}", list(seq[key].items()), gkey, step)
    names = K.grad_names(seq["actor"])
    check_stepped_twice(g, "seq_actor", [(k, seq["actor"][k]) for k in names], ("seq_ga0", "seq_ga1"), K.SEQ_ACTOR_LR)


def test_sac_entries_reject_bad_arguments_on_the_host():
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch: every refusal below comes before the first launch
    err = lambda: lib.dppo_last_error().decode()
    m = make_model("tiny", "fp32", "cpu")
    da, dq = m.network.net_desc(), m.critic.net_desc()
    N, F32 = 64, hip.PREC_F32
    cfg = m.network.sac_cfg(randn_clip=3.0)
    batch = lambda **kw: C.byref(hip.IdqlBatch(**dict(dict(obs=X, next_obs=X, actions=X, reward=X, terminated=X, inds=None, cap=N,
                                                           n_envs=1, head=0, count=N), **kw)))
    res = hip.NetDesc.from_buffer_copy(da)
    res.plain, res.hidden, res.n_blocks = 0, 128, 1
    odd = hip.NetDesc.from_buffer_copy(da)
    odd.out_dim = 7
    qres = hip.NetDesc.from_buffer_copy(dq)
    qres.plain, qres.hidden = 0, 128
    # ---- dppo_sac_sample
    ws = lib.dppo_sac_sample_workspace_bytes(C.byref(da), F32, N)
    assert ws > 0 and lib.dppo_sac_sample_workspace_bytes(C.byref(da), hip.PREC_BF16, N) > 0
    assert lib.dppo_sac_sample_workspace_bytes(C.byref(da), F32, 0) == -1 and "B out of range" in err()
    assert lib.dppo_sac_sample_workspace_bytes(C.byref(res), F32, N) == -1 and "plain trunk" in err()
    assert lib.dppo_sac_sample_workspace_bytes(C.byref(odd), F32, N) == -1 and "2 * Ta*Da" in err()
    assert lib.dppo_sac_sample_workspace_bytes(C.byref(da), 7, N) == -1

    def sample(a=da, prm=X, pk=X, cf=cfg, obs=X, B=N, act=X, w=X, wsb=ws):
        return lib.dppo_sac_sample(C.byref(a), F32, prm, pk, C.byref(cf) if cf is not None else None, obs, None, B, act, None, None, w,
                                   wsb, None)
    for kw in (dict(prm=None), dict(pk=None), dict(obs=None), dict(act=None), dict(w=None)):
        assert sample(**kw) == -1 and "null pointer" in err(), kw
    assert sample(cf=None) == -1 and "null cfg" in err()
    bad = copy.copy(cfg)
    bad.action_dim = 4
    assert sample(cf=bad) == -1 and "2 * Ta*Da" in err()
    bad = copy.copy(cfg)
    bad.squash = 2
    assert sample(cf=bad) == -1 and "0 or 1" in err()
    assert sample(B=0) == -1 and "B out of range" in err()
    assert sample(wsb=ws - 256) == -1 and "workspace too small" in err()
    # ---- dppo_sac_q_loss_fwd_bwd
    wq = lib.dppo_sac_q_loss_workspace_bytes(C.byref(dq), F32, 11, N)
    assert wq > 0 and lib.dppo_sac_q_loss_workspace_bytes(C.byref(dq), F32, 14, N) == -1 and "does not pair" in err()

    def qloss(q=dq, qp=X, k1=X, k2=X, tp=X, t1=X, t2=X, b=None, od=11, na=X, nl=X, al=X, N_=N, gamma=0.99, grad=X, st=X, w=X, wsb=wq):
        return lib.dppo_sac_q_loss_fwd_bwd(C.byref(q), F32, qp, k1, k2, tp, t1, t2, b or batch(), od, na, nl, al, N_, gamma, grad, st, w,
                                           wsb, None)
    for kw in (dict(qp=None), dict(k1=None), dict(k2=None), dict(tp=None), dict(t1=None), dict(t2=None), dict(na=None), dict(nl=None),
               dict(al=None), dict(grad=None), dict(st=None), dict(w=None)):
        assert qloss(**kw) == -1 and "null pointer" in err(), kw
    assert qloss(b=batch(reward=None)) == -1 and "null pointer in batch" in err()
    assert qloss(b=batch(head=N)) == -1 and "ring geometry" in err()
    assert qloss(N_=0) == -1 and "N out of range" in err()
    assert qloss(gamma=1.5) == -1 and "gamma" in err()
    assert qloss(od=14) == -1 and "does not pair" in err()
    assert qloss(wsb=wq - 256) == -1 and "workspace too small" in err()
    # ---- dppo_sac_actor_fwd_bwd
    wa = lib.dppo_sac_actor_workspace_bytes
    w = wa(C.byref(da), C.byref(dq), F32, 11, N)
    assert w > 0 and wa(C.byref(da), C.byref(dq), hip.PREC_BF16, 11, N) > 0

    def actor(a=da, q=dq, ap=X, ak=X, qp=X, k1=X, k2=X, cf=cfg, b=None, od=11, N_=N, al=X, grad=X, st=X, ws_=X, wsb=w):
        return lib.dppo_sac_actor_fwd_bwd(C.byref(a), C.byref(q), F32, ap, ak, qp, k1, k2, C.byref(cf) if cf is not None else None,
                                          b or batch(next_obs=None, actions=None, reward=None, terminated=None), od, N_, None, al, grad,
                                          st, None, None, None, None, ws_, wsb, None)
    for kw in (dict(ap=None), dict(ak=None), dict(qp=None), dict(k1=None), dict(k2=None), dict(al=None), dict(grad=None), dict(st=None),
               dict(ws_=None)):
        assert actor(**kw) == -1 and "null pointer" in err(), kw
    assert actor(cf=None) == -1 and "null cfg" in err()
    det = copy.copy(cfg)
    det.deterministic = 1
    assert actor(cf=det) == -1 and "deterministic" in err()
    assert actor(b=batch(obs=None)) == -1 and "null pointer in batch" in err()
    assert actor(b=batch(count=N - 1)) == -1 and "stored transitions" in err()
    for fn in (lambda **kw: actor(**kw), lambda N_=N, a=da, q=dq, od=11: wa(C.byref(a), C.byref(q), F32, od, N_)):
        assert fn(N_=0) == -1 and "N out of range" in err()
        assert fn(a=res) == -1 and "plain trunk" in err()
        assert fn(a=dq) == -1
        assert fn(q=qres) == -1 and "plain Q trunks" in err()
        assert fn(od=12) == -1 and "do not pair" in err()
    assert actor(wsb=w - 256) == -1 and "workspace too small" in err()
    # ---- dppo_sac_alpha_loss
    al = lambda lp=X, N_=N, la=X, te=-3.0, out=X: lib.dppo_sac_alpha_loss(lp, N_, la, te, out, None)
    for kw in (dict(lp=None), dict(la=None), dict(out=None)):
        assert al(**kw) == -1 and "null pointer" in err(), kw
    assert al(N_=0) == -1 and "N out of range" in err()
    assert al(te=float("nan")) == -1 and "target_entropy" in err()


def test_sac_model_has_no_cpu_path():
    from dppo_amd import hip
    m = make_model("tiny", "fp32", "cpu")
    with pytest.raises(hip.DppoHipError):
        m({"state": torch.zeros(2, 1, 11)})
    with pytest.raises(NotImplementedError, match="state observations"):
        m(cond={"state": torch.zeros(2, 1, 11), "rgb": torch.zeros(2, 1, 3, 8, 8)})


# ---------------------------------------------------------------------------------------------------------------- GPU
def dev_batch(case, n):
    return {k: v.to(DEV) for k, v in K.inputs(case, n).items()}


def alpha_dev(x=K.ALPHA):
    return torch.full((1,), float(x), dtype=torch.float64, device=DEV)


def run_sample(m, b, key="noise", **kw):
    a, logp = m({"state": b["obs"]}, get_logprob=True, noise=b[key], want_u=True, **kw)
    return a.reshape(len(a), -1).clone(), logp.clone(), m.last_u.clone()


def sample_errors(case, n, a, logp, ref):
    ea = (a.double().cpu() - ref["a"]).abs().max().item()
    el = (logp.double().cpu() - ref["logp"]).abs().max().item()
    print(f"{case}_{n}: sample off by {ea:.3e}, logp by {el:.3e} (|logp| up to {ref['logp'].abs().max():.2f})")
    return ea, el


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", PLAIN, ids=PLAIN_IDS)
def test_hip_sac_sample_fp32(case, n):
    """Actions within 2e-5 and logp within 2e-4 x AF of the float64 restatement (test_policy_head_edges' per-element Gaussian
    ceilings; logp is a SUM here), stochastic and deterministic; without the log-probability the same actions; Philox draws are
    reproducible from the seed bit for bit.  Given noise against Philox noise is an APPROXIMATE round trip, not the bit equality
    its wording suggests: there is no host Philox here, so the draws are recovered from the call's ``u_out`` as (u - mean) / scale
    with the float64 restatement's mean and scale, rounded to fp32 and fed back as given noise; the recovered draw is off from the
    kernel's by the fp32 error of mean and scale, so actions and log-probability are compared within the same 2e-5 and
    2e-4 x AF, not for equality."""
    m, b, r = make_model(case, "fp32", DEV), dev_batch(case, n), restated(case, n)
    af = K.shapes(case)[1] * K.shapes(case)[2]
    a, logp, u = run_sample(m, b)
    ea, el = sample_errors(case, n, a, logp, r["actor"])
    assert ea <= 2e-5 and el <= 2e-4 * af
    assert (u.double().cpu() - r["actor"]["u"]).abs().max() <= 2e-5
    assert torch.equal(m({"state": b["obs"]}, noise=b["noise"]).reshape(n, -1), a)
    ad, lpd, _ = run_sample(m, b, deterministic=True)
    ea, el = sample_errors(case, n, ad, lpd, r["det"])
    assert ea <= 2e-5 and el <= 2e-4 * af
    draws = []
    for _ in range(2):
        torch.manual_seed(5)
        pa, plp = m({"state": b["obs"]}, get_logprob=True, want_u=True)
        draws.append((pa.clone(), plp.clone(), m.last_u.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*draws))
    s = r["actor"]["sample"]
    z = ((draws[0][2].double().cpu() - s["mean"]) / s["scale"]).float().to(DEV)  # clamp(z): the draw as the head used it
    assert z.abs().max() <= K.RANDN_CLIP + 1e-3 and (n == 1 or z.std() > 0.5)
    ga, glp = m({"state": b["obs"]}, get_logprob=True, noise=z)
    assert (ga - draws[0][0]).abs().max() <= 2e-5 and (glp - draws[0][1]).abs().max() <= 2e-4 * af


@pytest.mark.gpu
def test_hip_sac_sample_saturated(golden):
    """tiny_sat: e_ref = the reference's own fp32 g27 value against the float64 restatement, max over the case; the call may be off
    from float64 by at most 2 e_ref (module docstring)."""
    (case, n), g = K.SAT_CASES[0], golden("g27_sac")
    m, b, r = make_model(case, "fp32", DEV), dev_batch(case, n), restated(case, n)
    a, logp, _ = run_sample(m, b)
    e_ref_a = np.abs(g[f"{case}_{n}_a"].astype(np.float64) - r["actor"]["a"].numpy()).max()
    e_ref_l = np.abs(g[f"{case}_{n}_logp"].astype(np.float64) - r["actor"]["logp"].numpy()).max()
    ea, el = sample_errors(case, n, a, logp, r["actor"])
    print(f"{case}_{n}: reference fp32 off by {e_ref_a:.3e} (sample), {e_ref_l:.3e} (logp)")
    assert torch.isfinite(logp).all()
    assert ea <= 2 * e_ref_a and el <= 2 * e_ref_l


def run_critic(m, b, replay=None, inds=None):
    src = replay if replay is not None else {"state": b["obs"]}
    loss = m.loss_critic(src, {"state": b["next_obs"]}, b["actions"], b["reward"], b["terminated"], K.GAMMA, alpha_dev(), inds=inds,
                         noise=b["noise_next"])
    return dict(loss=loss.detach().clone(), stats=m.last_stats.clone(), gq=m.critic.flat_grads().clone())


def run_actor(m, b, replay=None, inds=None):
    src = replay if replay is not None else {"state": b["obs"]}
    loss = m.loss_actor(src, alpha_dev(), inds=inds, noise=b["noise"])
    return dict(loss=loss.detach().clone(), stats=m.last_stats.clone(), ga=m.last_loss_grad.clone(), d_a=m.last_d_a.clone(),
                logp=m.last_logp.clone(), sel=m.last_sel.clone(), a=m.last_actions.clone())


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_sac_losses_fp32(golden, case, n):
    """Statistics by test_dql.stats_close, the rule of the QSM and DQL tests: 1e-5 of max(1, |ref|), relative only from |ref| = 1 up.
    The means below 1 come from O(1) terms that cancel (tiny_sat's actor loss is 0.052, the mean of -q_sel + alpha logp with
    |logp| up to 9): measured on MI355X, every statistic of every case is within 3.5e-6 of |ref| itself but that one, off by
    6.0e-7 = 1.2e-5 |ref|.  The temperature loss and its derivative (|ref| >= 1.9) are held to 1e-6 of |ref| (rel_close)."""
    g, name = golden("g27_sac"), f"{case}_{n}"
    m, b, r = make_model(case, "fp32", DEV), dev_batch(case, n), restated(case, n)
    # ---- critic: statistics within 1e-5, gradients by grad_violations' rule against the float64 restatement
    rc = run_critic(m, b)
    stats_close(rc["stats"].cpu().numpy(), r["critic"]["stats"], f"{name} critic")
    assert float(rc["loss"]) == float(rc["stats"][0].float())
    bad = grad_violations(r["critic"]["named"], by_name(named(m.critic, rc["gq"]), [k for k, _ in r["critic"]["named"]]))
    assert not bad, bad
    assert all(torch.equal(rc[k], v) for k, v in run_critic(m, b).items())
    # ---- actor: sel is the fixture's, statistics within 1e-5, d_a and every gradient on the call's own sel
    m.critic.flat_grads().fill_(7.0)
    q0 = m.critic.flat_params().clone()
    ra = run_actor(m, b)
    sel = ra["sel"].cpu().numpy().astype(bool)
    assert np.array_equal(sel.astype(np.uint8), g[f"{name}_sel"])
    stats_close(ra["stats"].cpu().numpy(), r["actor"]["stats"], f"{name} actor")
    assert float(ra["loss"]) == float(ra["stats"][0].float())
    if (case, n) not in K.SAT_CASES:
        af = K.shapes(case)[1] * K.shapes(case)[2]
        assert (ra["a"].double().cpu() - r["actor"]["a"]).abs().max() <= 2e-5
        assert (ra["logp"].double().cpu() - r["actor"]["logp"]).abs().max() <= 2e-4 * af
    check_on_own_sel(case, n, sel, named(m.network, ra["ga"]), ra["d_a"], name)
    assert bool((m.critic.flat_grads() == 7.0).all()) and torch.equal(m.critic.flat_params(), q0)  # the critic is only read
    again = run_actor(m, b)
    assert all(torch.equal(ra[k], again[k]) for k in ra), [k for k in ra if not torch.equal(ra[k], again[k])]
    # ---- temperature: value and derivative within 1e-6
    la = torch.tensor(K.SEQ_LOG_ALPHA, dtype=torch.float64, device=DEV, requires_grad=True)
    lt = m.loss_temperature({"state": b["obs"]}, la, K.target_entropy(case), noise=b["noise_t"])
    lt.backward()
    rel_close([m.last_alpha_out[0].item(), la.grad.item()], r["t"][:2], 1e-6, f"{name} temperature")
    # ---- a gathered call (indices into a ring with head != 0) equals the contiguous one bit for bit
    if n == 77:
        rp, inds = ring_of({k: b[k] for k in ("obs", "next_obs", "actions", "reward", "terminated")}, n)
        ring_c, ring_a = run_critic(m, b, replay=rp, inds=inds), run_actor(m, b, replay=rp, inds=inds)
        assert all(torch.equal(rc[k], ring_c[k]) for k in rc), [k for k in rc if not torch.equal(rc[k], ring_c[k])]
        assert all(torch.equal(ra[k], ring_a[k]) for k in ra), [k for k in ra if not torch.equal(ra[k], ring_a[k])]


@pytest.mark.gpu
def test_hip_sac_rows_do_not_depend_on_the_batch():
    """Rows 0..38 of a 39-row call against the same rows of the 77-row call: sample, log-probability and sel bit-equal; d_a carries
    1 / N, so N d_a agrees to fp32 rounding of that one division."""
    m, b = make_model("chunk", "fp32", DEV), dev_batch("chunk", 77)
    whole = run_actor(m, b)
    part = run_actor(m, {k: v[:39] for k, v in b.items()})
    for k in ("a", "logp", "sel"):
        assert torch.equal(part[k], whole[k][:39]), k
    x, y = 39.0 * part["d_a"].double(), 77.0 * whole["d_a"][:39].double()
    assert (x - y).abs().max() <= 1e-6 * y.abs().max()


@pytest.mark.gpu
def test_hip_sac_squash_off():
    """``GaussianModel.tanh_output=False`` (the head's squash flag 0: a = u, s = 1, no log-det term; in the tail du = -g / N) on
    chunk, N = 77: sample and log-probability within the fp32 bounds of the float64 restatement with the squash off, the actor loss
    by the rules of test_hip_sac_losses_fp32.  No fixture holds this case; ``sel`` is the float64 restatement's own, every
    |q1 - q2| ten times Q_CEIL from its edge (asserted here)."""
    case, n = "chunk", 77
    af = K.shapes(case)[1] * K.shapes(case)[2]
    m, b = make_model(case, "fp32", DEV, squash=False), dev_batch(case, n)
    ref = restate_actor_on(case, n, None, squash=False)
    assert (ref["q1"] - ref["q2"]).abs().min() >= 10 * K.Q_CEIL and 0 < ref["sel"].sum() < n
    assert torch.equal(ref["a"], ref["u"]) and not torch.equal(ref["a"], restated(case, n)["actor"]["a"])
    a, logp, u = run_sample(m, b)
    ea, el = sample_errors(case, n, a, logp, ref)
    assert torch.equal(a, u) and ea <= 2e-5 and el <= 2e-4 * af
    ra = run_actor(m, b)
    assert np.array_equal(ra["sel"].cpu().numpy().astype(bool), ref["sel"])
    stats_close(ra["stats"].cpu().numpy(), ref["stats"], "squash off actor")
    assert (ra["a"].double().cpu() - ref["a"]).abs().max() <= 2e-5 and (ra["logp"].double().cpu() - ref["logp"]).abs().max() <= 2e-4 * af
    order = [k for k, _ in ref["named"]]
    bad = grad_violations([("d_a", ref["d_a"])] + ref["named"], [("d_a", ra["d_a"])] + by_name(named(m.network, ra["ga"]), order))
    assert not bad, bad


def agent_cfg(tmp_path, **train):
    cfg = copy.deepcopy(load_config(SHIPPED)[SAC_CFG])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=4, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.pop("wandb", None)
    cfg.model.update(device=DEV)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = "fp32"
    cfg.train.update(dict(n_train_itr=6, n_explore_steps=2, n_steps=1, batch_size=8, critic_replay_ratio=8, actor_replay_ratio=4,
                          buffer_size=64, val_freq=100, save_model_freq=100, log_freq=1), **train)
    return cfg


@pytest.mark.gpu
def test_hip_sac_agent_minibatch_is_the_recorded_sequence(golden, tmp_path):
    """One fp32 ``update_minibatch`` on cheetah, N = 77, against the sequence the reference recorded: critic step, Polyak, two
    actor + temperature steps, ``log_alpha`` included."""
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    from dppo_amd.util.optim import FlatAdamW
    from dppo_amd.util.replay import DeviceReplay
    g, case, n = golden("g27_sac"), "cheetah", 77
    agent = TrainSACAgent(agent_cfg(tmp_path, n_train_itr=0, target_ema_rate=K.SEQ_TAU))
    m = agent.model = make_model(case, "fp32", DEV)
    agent.gamma, agent.target_entropy = K.GAMMA, K.target_entropy(case)
    agent.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=K.SEQ_LR, weight_decay=0)
    agent.actor_optimizer = FlatAdamW(m.network.flat_params(), lr=K.SEQ_ACTOR_LR, weight_decay=0)
    agent.log_alpha = torch.tensor(K.SEQ_LOG_ALPHA, dtype=torch.float64, device=DEV, requires_grad=True)
    agent.log_alpha_optimizer = torch.optim.Adam([agent.log_alpha], lr=K.SEQ_LR)
    b = dev_batch(case, n)
    od, ta, da = K.shapes(case)
    rp = agent.replay = DeviceReplay(n, 1, od, ta * da, device=DEV)
    for dst, key in ((rp.obs, "obs"), (rp.next_obs, "next_obs"), (rp.actions, "actions"), (rp.reward, "reward"), (rp.terminated, "terminated")):
        dst.copy_(b[key].reshape(dst.shape))
    rp.steps = n
    seen = []
    inner = m.loss_actor
    m.loss_actor = lambda *a, **k: seen.append(inner(*a, **k).detach().clone()) or seen[-1]
    lc, la, lt = agent.update_minibatch(torch.arange(n, device=DEV), sample_noise=b["noise_next"], actor_noise=[b["noise"], b["noise2"]],
                                        temp_noise=[b["noise_t"], b["noise_t2"]])
    print(f"seq: critic {float(lc)!r} ref {float(g['seq_c_loss'])!r}; actor {[float(x) for x in seen]} ref {g['seq_a_loss']}; "
          f"temperature {float(lt)!r} ref {g['seq_t_loss']}; log_alpha {float(agent.log_alpha.detach())!r} ref {g['seq_log_alpha']}")
    np.testing.assert_allclose([float(lc)] + [float(x) for x in seen] + [float(lt)],
                               [float(g["seq_c_loss"])] + list(g["seq_a_loss"]) + [float(g["seq_t_loss"][1])], rtol=2e-4, atol=2e-5)
    assert abs(float(agent.log_alpha.detach()) - float(g["seq_log_alpha"][1])) <= 1e-6
    check_grads_fp32(g, "seq_gq", named(m.critic, m.critic.flat_grads()))
    check_grads_fp32(g, "seq_ga1", named(m.network, m.last_loss_grad))
    for key, net, gkey, step in (("seq_q", m.critic, "seq_gq", K.SEQ_LR), ("seq_target", m.target_critic, "seq_gq", K.SEQ_LR * K.SEQ_TAU)):
        check_stepped(g, key, list(net.named_parameters()), gkey, step)
    check_stepped_twice(g, "seq_actor", [(k, p) for k, p in m.network.named_parameters() if p.requires_grad], ("seq_ga0", "seq_ga1"),
                        K.SEQ_ACTOR_LR)


@pytest.mark.gpu
def test_hip_sac_agent_runs(tmp_path):
    """The shipped cfg shrunk (4 envs, batch 8, 2 exploration iterations, 6 iterations): iterations 3..5 update the critic, 4 the
    actor and the temperature too; losses are finite and every network moves; a checkpoint round-trips."""
    from dppo_amd.agent.finetune.train_sac_agent import TrainSACAgent
    agent = TrainSACAgent(agent_cfg(tmp_path))
    m = agent.model
    assert (agent.critic_update_freq, agent.actor_update_freq, agent.n_explore_steps) == (1, 2, 2)
    assert agent.target_entropy == -6 and float(agent.log_alpha.detach()) == 0.0
    actor0, critic0, target0 = (x.flat_params().clone() for x in (m.network, m.critic, m.target_critic))
    calls = []
    inner = agent.update_minibatch
    agent.update_minibatch = lambda inds, **kw: calls.append((agent.itr, kw["update_actor"])) or inner(inds, **kw)
    res = agent.run()
    assert calls == [(3, False), (4, True), (5, False)]
    assert [r["itr"] for r in res] == list(range(6)) and res[-1]["step"] == 6 * 4
    assert all(np.isfinite(r["loss_critic"]) for r in res[3:]) and np.isfinite(res[4]["loss_actor"]) and np.isfinite(res[5]["alpha"])
    for net, before in ((m.network, actor0), (m.critic, critic0), (m.target_critic, target0)):
        assert not torch.equal(net.flat_params(), before) and bool(torch.isfinite(net.flat_params()).all())
    assert float(agent.log_alpha.detach()) != 0.0
    data = torch.load(os.path.join(str(tmp_path), "checkpoint", "state_5.pt"), weights_only=True)
    assert len(data["model"]) == 34
    other = TrainSACAgent(agent_cfg(tmp_path, n_train_itr=0))
    other.load(5)
    for a, b in ((other.model.network, m.network), (other.model.critic, m.critic), (other.model.target_critic, m.target_critic)):
        assert torch.equal(a.flat_params(), b.flat_params())


# ---------------------------------------------------------------------------------------------------------------- bf16
def bf16_figures(case, n):
    """Runs the bf16 actor call; returns (the yardstick's errors e_y, the call's errors, rows whose sel differs from the fp32
    restatement's), all against the fp32-operand restatement on the call's own sel."""
    m, b = make_model(case, "bf16", DEV), dev_batch(case, n)
    res = run_actor(m, b)
    sel = res["sel"].cpu().numpy().astype(bool)
    fp32 = restate_actor_on(case, n, sel, dtype=torch.float32)
    yard = restate_actor_on(case, n, sel, bf16=True, dtype=torch.float32)
    order = [k for k, _ in fp32["named"]]
    call = dict(loss=res["loss"], d_a=res["d_a"], named=by_name(named(m.network, res["ga"]), order))
    return rel_errors(fp32, yard), rel_errors(fp32, call), int((sel != restated(case, n)["actor"]["sel"]).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_sac_bf16_within_twice_the_rounding_yardstick(case, n):
    """Every case, N = 1 included: there no rounding of a row of d_out or of the chain's dz is averaged down in a bias sum."""
    e_y, e_c, flips = bf16_figures(case, n)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    print(f"{case}_{n} bf16: yardstick loss {e_y['loss']:.3e} d_a {e_y['d_a']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss "
          f"{e_c['loss']:.3e} d_a {e_c['d_a']:.3e} 1-cos {e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} "
          f"against {e_y['per'][worst]:.3e}; sel differs from fp32's in {flips} rows")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["d_a"] <= 2 * e_y["d_a"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])
