"""DQL fine-tuning (reference model/diffusion/diffusion_dql.py, agent/finetune/train_dql_diffusion_agent.py): the 8 shipped DQL cfgs
resolve, ``DQLDiffusion`` carries the reference's state dict, both new C ABI entries check their arguments, and the plain-torch
restatement of tests/golden/make_golden_dql_cases.py reproduces the g26 fixture the reference wrote (CPU).  On the GPU the actor loss
differentiated through the K-step sampling chain is held to the reference's masks, losses and statistics and -- for d loss / d action
and every parameter gradient -- to the restatement evaluated ON THE CALL'S OWN chain and masks (so an x0 that lands on the other
side of the clamp's edge can neither hide nor cause a failure), and to g26 directly where the masks agree.  ReLU's derivative has
the same kind of edge at 0: check_on_own_chain hands the few gates within make_golden_dql_cases.RELU_TIE of it over as well.

Chains.  g26 stores the reference's chain in full for make_golden_dql_cases.FULL_CHAINS only (the file stays below g25's size);
for the other cases the "given chain" is the restatement's, which the CPU test pins to the reference's stored entries at 1e-5.

bf16.  No tolerance is fixed: the yardstick is the restatement with every Linear's operands rounded to bf16
(make_golden_dql_cases.bf16_linears), evaluated on the chain and masks the bf16 call returned; with e_y its error against the fp32
restatement on the same chain and masks, the call may be off by at most 2 e_y (loss, d_a, per tensor, 1 - cosine).
tools/dql_parity_report.py writes the measured figures to profiles/dql_parity.json; nothing here reads that file.
"""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from dppo_amd.cfg.loader import Cfg, get_class, instantiate, load_config
from tests.golden import make_golden_dql_cases as K
from tests.golden import make_golden_qsm_cases as Q
from tests.test_idql import check_grads_fp32
from tests.test_qsm import close_to_fixture, make_q, named_grads, ring_of

T = torch.from_numpy
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = os.path.join(HERE, "golden", "shipped_dql_cfgs.json")
HOPPER_CFG = "gym/finetune/hopper-v2/ft_dql_diffusion_mlp.yaml"
IDS = [f"{c}_{n}" for c, n in K.CASES]


def ref_masks(g, case, n):
    od, ta, da, steps = K.shapes(case)
    return np.unpackbits(g[f"{case}_{n}_masks"])[:n * steps * ta * da].reshape(n, steps, ta * da).astype(bool)


@functools.lru_cache(maxsize=None)
def restated(case, n):
    """The restatement of one case with its own chain and masks: computed once, shared, never modified."""
    return K.loss_actor(Q.leaf(Q.actor_params(K.net_of(case))), Q.twin_params(K.net_of(case)), case, K.inputs(case, n))


def given_chain(g, case, n):
    """The chain a 'chain given' run consumes: the reference's where g26 stores it in full, else the restatement's."""
    key = f"{case}_{n}_chain"
    return T(g[key].copy()) if key in g else restated(case, n)["chain"].clone()


def restate_on(case, n, chain, masks, bf16=False, gates=None):
    """gates: a make_golden_dql_cases.relu_gates context to evaluate under (None: a fresh one that forces nothing)."""
    a = Q.leaf(Q.actor_params(K.net_of(case)))
    od, ta, da, steps = K.shapes(case)
    args = (a, Q.twin_params(K.net_of(case)), case, K.inputs(case, n))
    kw = dict(chains=chain.reshape(n, steps + 1, ta, da), masks=masks)
    with gates if gates is not None else K.relu_gates() as rg:
        if bf16:
            with K.bf16_linears():
                res = K.loss_actor(*args, **kw)
        else:
            res = K.loss_actor(*args, **kw)
    res["named"], res["near_zero"] = list(zip(a, res["grads"])), rg.near_zero()
    return res


def grad_violations(want, got):
    """check_grads_fp32's rule with another tensor in the fixture's place: rtol 2e-3, atol 2e-4 ||ref|| / sqrt(size) + 1e-7 per
    entry, and the norms within 2e-4.  Returns [(tensor, entries outside the rule, worst excess, norm outside?)] of the tensors
    that miss it."""
    bad = []
    for (k, r), (k2, x) in zip(want, got):
        r, x = r.detach().cpu().numpy().astype(np.float64), x.detach().cpu().numpy().astype(np.float64).reshape(r.shape)
        ref_n = float(np.linalg.norm(r))
        atol = 2e-4 * max(ref_n, 1e-8) / np.sqrt(r.size) + 1e-7
        over = np.abs(x - r) - (atol + 2e-3 * np.abs(r))
        norm_off = abs(float(np.linalg.norm(x)) - ref_n) > max(2e-4 * ref_n, 1e-7)
        if (over > 0).any() or norm_off:
            bad.append((k, int((over > 0).sum()), float(over.max()), norm_off))
    return bad


def check_on_own_chain(case, n, chain, masks, named, d_a, what):
    """d_a and every gradient of a run against the restatement on the run's chain and masks, by check_against's rule on EVERY
    entry.  Where that misses and the network is a ReLU one, the yardstick's gates below RELU_TIE (the reasoning stands beside
    that constant) are tried on their other side, nearest to zero first, each kept if it lowers the count of entries outside the
    rule: the run must meet the whole rule for ONE assignment of those few gates, as it must for one set of clamp masks."""
    got = [("d_a", d_a)] + list(named)
    ref = restate_on(case, n, chain, masks)
    bad = grad_violations([("d_a", ref["d_a"])] + ref["named"], got)
    if not bad or Q.actor_spec(K.net_of(case)).activation != "ReLU":
        assert not bad, (what, bad)
        return
    count = lambda b: sum(x[1] + int(x[3]) for x in b)
    print(f"{what}: {count(bad)} entries outside the rule {bad}; {len(ref['near_zero'])} ReLU gates below {K.RELU_TIE:g}")
    force = {}
    for z, where, gate in ref["near_zero"]:
        trial = dict(force)
        trial[where] = not gate
        res = restate_on(case, n, chain, masks, gates=K.relu_gates(trial))
        now = grad_violations([("d_a", res["d_a"])] + res["named"], got)
        print(f"{what}: gate {where} (|z| {z:.2e}) on its other side: {count(now)} entries outside the rule")
        if count(now) < count(bad):
            force, bad = trial, now
        if not bad:
            return
    assert not bad, (what, bad, force)


def stats_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: stats {got} ref {ref} err {err.max():.2e}")
    assert err.max() <= 1e-5, (what, got, ref)


def check_stepped(g, key, named, gkey, step):
    """Stepped weights against the recorded ones (test_hip_qsm_agent_minibatch_is_the_recorded_sequence's rule).  AdamW's first
    step is lr * g / (|g| + eps): an entry whose gradient is off by dg moves off by lr * dg / (|g| + eps), with dg from the gradient
    rule (rtol 2e-3, the tensor's atol) -- and by at most 2 lr whatever the gradient; the target moves by tau times the critic's
    step.  Plus one ulp-class term for the weight itself; and nearly all entries are tight."""
    for k, p in named:
        x = p.detach().cpu().numpy()
        if f"{key}_{k}" in g:
            ref, xs, gref = g[f"{key}_{k}"], x, g[f"{gkey}_{k}"]
            gn = float(np.linalg.norm(gref))
        else:
            ref, xs, gref, gn = g[f"{key}_{k}__sub"], x.reshape(-1)[::61], g[f"{gkey}_{k}__sub"], float(g[f"{gkey}_{k}__norm"])
        atol_g = 2e-4 * max(gn, 1e-8) / np.sqrt(x.size) + 1e-7
        tol = step * np.minimum(2.0, 2e-3 + atol_g / (np.abs(gref) + 1e-8)) + 1e-6 * np.abs(ref) + 1e-7
        assert (np.abs(xs - ref) <= tol).all(), (key, k, float(np.abs(xs - ref).max()))
        assert (np.abs(xs - ref) <= step * 1e-2 + 1e-6 * np.abs(ref) + 1e-7).mean() > 0.99, (key, k)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_every_shipped_dql_cfg_resolves():
    from dppo_amd import hip
    from dppo_amd.agent.finetune.train_dql_diffusion_agent import TrainDQLDiffusionAgent
    from dppo_amd.model.common.critic import CriticObsAct
    from dppo_amd.model.diffusion.diffusion_dql import DQLDiffusion
    lib = hip.load()
    cfgs = load_config(SHIPPED)
    assert len(cfgs) == 8 and "gym/scratch/hopper-v2/dql_diffusion_mlp.yaml" in cfgs
    assert sum(p.endswith("ft_dql_diffusion_mlp.yaml") for p in cfgs) == 7
    for p in sorted(cfgs):
        cfg = cfgs[p]
        assert get_class(cfg._target_) is TrainDQLDiffusionAgent, p
        assert get_class(cfg.model._target_) is DQLDiffusion, p
        assert get_class(cfg.model.critic._target_) is CriticObsAct, p
        assert cfg.act_steps == cfg.horizon_steps and cfg.train.eta > 0, p
        m = instantiate(cfg.model, network_path=None)
        assert type(m) is DQLDiffusion and m.actor is m.network and m.critic_target is not m.critic, p
        da, dq = m.actor.net_desc(), m.critic.net_desc()
        od = cfg.obs_dim * cfg.cond_steps
        assert dq.plain == 1 and dq.in_dim == od + cfg.action_dim * cfg.act_steps and da.plain == 0, p
        N = int(cfg.train.batch_size)
        for prec in (hip.PREC_F32, hip.PREC_BF16):
            assert lib.dppo_dql_actor_workspace_bytes(C.byref(da), C.byref(dq), prec, od, N, int(cfg.denoising_steps)) > 0, \
                (p, lib.dppo_last_error())
            assert lib.dppo_qsm_q_loss_workspace_bytes(C.byref(dq), prec, od, N) > 0, p


def make_model(case, prec, device):
    from dppo_amd.model.diffusion.diffusion_dql import DQLDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    net = K.net_of(case)
    od, ta, da, steps = K.shapes(case)
    a = Q.actor_spec(net)
    actor = DiffusionMLP(da, ta, od, time_dim=a.time_dim, mlp_dims=list(a.mlp_dims), activation_type=a.activation,
                         residual_style=True, precision=prec)
    actor.load_state_dict(Q.actor_params(net), strict=True)
    q = make_q(net, prec)
    q.load_state_dict(Q.twin_params(net), strict=True)
    m = DQLDiffusion(actor=actor, critic=q, horizon_steps=ta, obs_dim=od, action_dim=da, device=device, denoising_steps=steps,
                     **K.SAMPLING_KW, **K.model_kw(case))
    m.critic_target.load_state_dict(Q.twin_params(net, Q.TARGET_EPS), strict=True)
    return m


def test_dql_state_dict_is_the_references(golden):
    g = golden("g26_dql")
    sd = make_model("hopper", "fp32", "cpu").state_dict()
    assert list(sd) == [str(k) for k in g["state_dict_keys"]]
    assert [",".join(str(int(x)) for x in v.shape) for v in sd.values()] == [str(s) for s in g["state_dict_shapes"]]
    assert {k.split(".")[0] for k in sd} == {"network", "actor", "critic", "critic_target"}


@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_restatement_reproduces_the_reference_fixture(golden, case, n):
    """Losses and statistics to 1e-5 of max(1, |ref|), the chain to 1e-5 of its largest entry, the masks EQUAL, d_a and every
    gradient by check_grads_fp32's rule; with the reference's masks passed in the restatement is bit-equal to itself; the near-tie
    list is what the restatement's own x0_raw gives and holds at most 0.1 % of the elements."""
    g, name, res = golden("g26_dql"), f"{case}_{n}", restated(case, n)
    stats_close(res["stats"], g[f"{name}_stats"], name)
    assert abs(float(res["loss"]) - float(g[f"{name}_loss"])) <= 1e-5 * max(1.0, abs(float(g[f"{name}_loss"])))
    close_to_fixture(g, f"{name}_chain", res["chain"], "chain")
    masks = ref_masks(g, case, n)
    assert np.array_equal(res["masks"], masks), int((res["masks"] != masks).sum())
    a = Q.actor_params(K.net_of(case))
    check_grads_fp32(g, name, [("d_a", res["d_a"])])
    check_grads_fp32(g, f"{name}_ga", list(zip(a, res["grads"])))
    ties = g[f"{name}_ties"]
    clip = K.model_kw(case)["denoised_clip_value"]
    assert ties.size <= K.NEAR_TIE_CAP * masks.size
    mine = K.near_ties(res["x0_raw"], K.shapes(case)[3], clip)
    assert len(set(mine.tolist()) ^ set(ties.tolist())) <= 2, (mine, ties)  # (an element at the edge of the near-tie band itself)
    if n == 77:
        again = K.loss_actor(Q.leaf(a), Q.twin_params(K.net_of(case)), case, K.inputs(case, n), masks=masks)
        assert torch.equal(again["loss"], res["loss"]) and torch.equal(again["d_a"], res["d_a"])
        assert all(torch.equal(x, y) for x, y in zip(again["grads"], res["grads"]))
        assert np.array_equal(again["masks"], masks) and np.array_equal(again["x0_raw"], res["x0_raw"])


def test_restatement_reproduces_the_recorded_sequence(golden):
    g = golden("g26_dql")
    seq = K.restate_sequence(K.critic_batch(77))
    close_to_fixture(g, "seq_c_loss", seq["c_loss"], "seq")
    close_to_fixture(g, "seq_a_loss", seq["a_loss"], "seq")
    assert float(g["seq_a_loss"]) != float(g["hopper_77_loss"])  # the stepped critic moved the seed
    for key in ("gq", "ga"):
        for k, v in seq[key].items():
            close_to_fixture(g, f"seq_{key}_{k}", v, "seq")
    # the stepped weights: AdamW's first step divides by |g| + 1e-8, so 1e-5 of the GRADIENT is not 1e-5 of the step where |g| is tiny
    for key, gkey, step in (("q", "seq_gq", K.SEQ_LR), ("actor", "seq_ga", K.SEQ_ACTOR_LR), ("target", "seq_gq", K.SEQ_LR * K.SEQ_TAU)):
        check_stepped(g, f"seq_{key}", list(seq[key].items()), gkey, step)


def test_dql_entries_reject_bad_arguments_on_the_host():
    from dppo_amd import hip
    lib = hip.load()
    X = 4096  # a non-null address no call may touch: every refusal below comes before the first launch
    err = lambda: lib.dppo_last_error().decode()
    m = make_model("hopper", "fp32", "cpu")
    da, dq, dres = m.actor.net_desc(), m.critic.net_desc(), make_q("hopper_res").net_desc()
    N, F32, steps = 64, hip.PREC_F32, 20
    wsq = lib.dppo_dql_actor_workspace_bytes
    w = wsq(C.byref(da), C.byref(dq), F32, 11, N, steps)
    assert w > 0 and wsq(C.byref(da), C.byref(dq), hip.PREC_BF16, 11, N, steps) > 0
    assert wsq(C.byref(da), C.byref(dq), F32, 11, N, 10) < w  # the workspace grows with the chain
    cfg = C.byref(m.diffusion_cfg())
    batch = lambda **kw: C.byref(hip.IdqlBatch(**dict(dict(obs=X, next_obs=None, actions=None, reward=None, terminated=None, inds=None,
                                                           cap=N, n_envs=1, head=0, count=N), **kw)))

    def call(a=da, q=dq, ap=X, ak=X, qp=X, k1=X, k2=X, cf=cfg, ts=X, st=steps, b=None, od=11, N_=N, ch=X, nz=X, tb=X, sa=X, sb=X,
             eta=1.0, which=0, grad=X, stats=X, ws=X, wsb=w):
        return lib.dppo_dql_actor_fwd_bwd(C.byref(a), C.byref(q), F32, ap, ak, qp, k1, k2, cf, ts, st, b or batch(), od, N_, ch, nz, tb,
                                          sa, sb, eta, which, grad, stats, None, None, ws, wsb, None)
    for kw in (dict(ap=None), dict(ak=None), dict(qp=None), dict(k1=None), dict(k2=None), dict(cf=None), dict(ts=None), dict(ch=None),
               dict(nz=None), dict(tb=None), dict(sa=None), dict(sb=None), dict(grad=None), dict(stats=None), dict(ws=None)):
        assert call(**kw) == -1 and "null pointer" in err(), kw
    assert call(b=batch(obs=None)) == -1 and "null pointer in batch" in err()
    assert call(b=batch(head=N)) == -1 and "ring geometry" in err()
    assert call(b=batch(count=N - 1)) == -1 and "stored transitions" in err()
    for fn in (lambda **kw: call(**kw), lambda N_=N, st=steps, a=da, q=dq, od=11: wsq(C.byref(a), C.byref(q), F32, od, N_, st)):
        assert fn(N_=0) == -1 and "N out of range" in err()
        for st in (0, 1025):
            assert fn(st=st) == -1 and "outside [1, 1024]" in err()
        assert fn(a=dq) == -1 and "actor descriptor" in err()
        assert fn(q=dres) == -1 and "plain Q trunks" in err()
        assert fn(od=12) == -1 and "do not pair" in err()
        bad = hip.NetDesc.from_buffer_copy(da)
        bad.plain, bad.hidden = 1, 512
        assert fn(a=bad) == -1
    for which in (-1, 2):
        assert call(which=which) == -1 and "which=" in err()
    for eta in (float("nan"), float("inf")):
        assert call(eta=eta) == -1 and "eta" in err()
    assert call(wsb=w - 256) == -1 and "workspace too small" in err()
    assert wsq(C.byref(da), C.byref(dq), 7, 11, N, steps) == -1


def test_dql_model_refuses_what_the_reference_refuses():
    from dppo_amd import hip
    from dppo_amd.model.diffusion.diffusion_dql import DQLDiffusion
    from dppo_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    mk = lambda critic=None, **kw: DQLDiffusion(actor=DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=True),
                                                critic=critic or make_q("hopper"), horizon_steps=4, obs_dim=11, action_dim=3,
                                                device="cpu", denoising_steps=20, **kw)
    with pytest.raises(AssertionError, match="DDIM"):
        mk(use_ddim=True, ddim_steps=5)
    with pytest.raises(ValueError, match="twin critic"):
        mk(critic=make_q("hopper", double_q=False))
    m = mk()
    with pytest.raises(NotImplementedError, match="act_steps == horizon_steps"):
        m.loss_actor({"state": torch.zeros(2, 1, 11)}, 1.0, 2)
    with pytest.raises(NotImplementedError, match="state observations"):
        m(cond={"state": torch.zeros(2, 1, 11), "rgb": torch.zeros(2, 1, 3, 8, 8)})
    with pytest.raises(hip.DppoHipError):  # no CPU fallback
        m.loss_actor({"state": torch.zeros(2, 1, 11)}, 1.0, 4)


# ---------------------------------------------------------------------------------------------------------------- GPU
def run_actor(m, case, n, chain=None, rows=slice(None), replay=None, inds=None, noise=None):
    b = K.inputs(case, n)
    src = replay if replay is not None else {"state": b["obs"][rows].to(DEV)}
    loss = m.loss_actor(src, K.ETA, K.shapes(case)[1], inds=inds, noise=noise, noise_bc=b["noise_bc"][rows].to(DEV),
                        t_bc=b["t_bc"][rows].to(DEV), which=K.which(case), chains=None if chain is None else chain[rows].to(DEV),
                        want_masks=True)
    return dict(loss=loss.detach().clone(), stats=m.last_stats.clone(), d_a=m.last_d_a.clone(), masks=m.last_masks.clone(),
                ga=m.last_loss_grad.clone(), chain=m.last_chains.clone())


def check_run(g, case, n, m, res, e2e=False):
    """One fp32 run against the reference (masks outside the near-tie list, statistics) and against the restatement on the run's
    own chain and masks (d_a, every gradient); against g26's gradients too where the masks are the reference's."""
    name = f"{case}_{n}"
    masks, want = res["masks"].cpu().numpy().astype(bool), ref_masks(g, case, n)
    diff = np.flatnonzero(masks != want)
    print(f"{name}: {diff.size} mask elements differ from the reference ({g[name + '_ties'].size} near ties)")
    assert set(diff.tolist()) <= set(g[f"{name}_ties"].tolist()), diff
    stats_close(res["stats"].cpu().numpy(), g[f"{name}_stats"], name)
    assert float(res["loss"]) == float(res["stats"][0].float())
    check_on_own_chain(case, n, res["chain"].cpu(), masks, named_grads(m.actor, res["ga"]), res["d_a"], name)
    if diff.size == 0 and not e2e:
        check_grads_fp32(g, name, [("d_a", res["d_a"])])
        check_grads_fp32(g, f"{name}_ga", named_grads(m.actor, res["ga"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_dql_chain_given_fp32(golden, case, n):
    g = golden("g26_dql")
    m, chain = make_model(case, "fp32", DEV), given_chain(g, case, n)
    m.critic.flat_grads().fill_(7.0)
    q0 = m.critic.flat_params().clone()
    res = run_actor(m, case, n, chain)
    check_run(g, case, n, m, res)
    assert bool((m.critic.flat_grads() == 7.0).all()) and torch.equal(m.critic.flat_params(), q0)  # the critic is only read
    again = run_actor(m, case, n, chain)
    assert all(torch.equal(res[k], again[k]) for k in res), [k for k in res if not torch.equal(res[k], again[k])]
    if n == 77:  # a gathered call (indices into a ring with head != 0) equals the contiguous one bit for bit
        b = K.inputs(case, n)
        od, ta, da, _ = K.shapes(case)
        rp, inds = ring_of(dict(obs=b["obs"].to(DEV), next_obs=b["obs"].to(DEV), actions=torch.zeros(n, ta * da, device=DEV),
                                reward=torch.zeros(n, device=DEV), terminated=torch.zeros(n, device=DEV)), n)
        ring = run_actor(m, case, n, chain, replay=rp, inds=inds)
        assert all(torch.equal(res[k], ring[k]) for k in res), [k for k in res if not torch.equal(res[k], ring[k])]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["scratch", "hopper", "hopper_final", "hopper_k1", "transport"])
def test_hip_dql_end_to_end_fp32(golden, case):
    """chains=None: the persistent sampler draws the chain from the recipe's noise -- within 1e-5 of the reference's, the loss
    within 1e-5 --, and the gradients are the restatement's on the call's own chain and masks.

    Measured on MI355X: scratch, hopper_final, hopper_k1 and transport meet the rule on every entry as the restatement stands.
    ``hopper`` does with one ReLU gate on its other side: with the restatement's own gates 65 of the 262,144 entries of
    mlp_mean.layers.1.l1.weight -- one row -- are off by up to 2.6e-6 against an atol of 2.7e-7 while d_a, the masks (0 differ) and
    the statistics (2.3e-7) hold (check_on_own_chain says how such a gate is handed over)."""
    g, n = golden("g26_dql"), 77
    m = make_model(case, "fp32", DEV)
    res = run_actor(m, case, n, noise=K.inputs(case, n)["noise"].to(DEV))
    close_to_fixture(g, f"{case}_{n}_chain", res["chain"].reshape(n, -1, res["chain"].shape[-1]), "sampled chain")
    check_run(g, case, n, m, res, e2e=True)
    assert torch.equal(m.forward_train({"state": K.inputs(case, n)["obs"].to(DEV)}, noise=K.inputs(case, n)["noise"].to(DEV)).reshape(n, -1),
                       res["chain"][:, -1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hopper", "transport"])
def test_hip_dql_rows_do_not_depend_on_the_batch(golden, case):
    """Rows 0..38 of a 39-row call against the same rows of the 77-row call.  The masks are bit-equal.  d_a carries the batch's
    own factors -- 2 / (N AF) of the BC mean and -eta / (N mean|q_j|) of the seed -- so the two calls cannot agree bit for bit
    as they stand; what is bit-equal is d_a of rows 0..38 between two 77-ROW calls whose other rows differ (eta = 0: the seed's
    scale is a mean over all rows), and N * d_a between the 39-row and the 77-row call agrees to fp32 rounding: every element is
    rounded once per GEMM epilogue and link, (K + 1) (2 n_blocks + 3) <= 105 times at 2^-24 of the running magnitude, so
    |diff| <= 1e-5 * max|N d_a| (6e-6 by that count)."""
    g = golden("g26_dql")
    m, chain, b = make_model(case, "fp32", DEV), given_chain(g, case, 77), K.inputs(case, 77)
    whole, part = run_actor(m, case, 77, chain), run_actor(m, case, 77, chain, rows=slice(0, 39))
    assert torch.equal(part["masks"], whole["masks"][:39])

    def d_a(rows, eta=0.0):
        m.loss_actor({"state": b["obs"][rows].to(DEV)}, eta, K.shapes(case)[1], noise_bc=b["noise_bc"][rows].to(DEV),
                     t_bc=b["t_bc"][rows].to(DEV), which=0, chains=chain[rows].to(DEV))
        return m.last_d_a.clone()
    other = torch.cat([torch.arange(39), torch.arange(76, 38, -1)])  # the same first 39 rows, the rest in another order
    assert torch.equal(d_a(other)[:39], d_a(slice(None))[:39])
    a39, a77 = (39.0 * d_a(slice(0, 39)).double()).cpu().numpy(), (77.0 * d_a(slice(None)).double()[:39]).cpu().numpy()
    print(f"{case}: max |39 d_a(39 rows) - 77 d_a(77 rows)| {np.abs(a39 - a77).max():.3e} of {np.abs(a77).max():.3e}")
    assert np.abs(a39 - a77).max() <= 1e-5 * np.abs(a77).max()


def agent_cfg(tmp_path, **train):
    cfg = copy.deepcopy(load_config(SHIPPED)[HOPPER_CFG])
    cfg.update(device=DEV, seed=42, logdir=str(tmp_path), env=Cfg(n_envs=8, name="synthetic", max_episode_steps=5, reset_at_iteration=False))
    cfg.pop("wandb", None)
    cfg.model.update(device=DEV, network_path=None)
    for node in (cfg.model.actor, cfg.model.critic):
        node["precision"] = "fp32"
    cfg.train.update(dict(n_train_itr=3, n_critic_warmup_itr=1, n_steps=4, batch_size=16, replay_ratio=2, buffer_size=3, val_freq=100,
                          force_train=True, save_model_freq=100), **train)
    return cfg


@pytest.mark.gpu
def test_hip_dql_agent_runs_the_reference_update_order(tmp_path):
    """hopper cfg shrunk (8 envs, 4 steps, batch 16, replay_ratio 2, 3 iterations, 1 warm-up): during the warm-up iteration the
    actor's loss and gradient are computed but its parameters do not move, afterwards they do; after every minibatch the target is
    the Polyak recurrence of its previous value and the freshly stepped critic; rewards are scaled; a checkpoint round-trips."""
    from dppo_amd.agent.finetune.train_dql_diffusion_agent import TrainDQLDiffusionAgent
    agent = TrainDQLDiffusionAgent(agent_cfg(tmp_path))
    m = agent.model
    assert agent.replay.cap == 3 and agent.eta == 1.0 and agent.scale_reward_factor == 0.01 and agent.target_ema_rate == 0.005
    actor0, critic0 = m.actor.flat_params().clone(), m.critic.flat_params().clone()
    actor_after, polyak_ok, warm = {}, [], []
    inner = agent.update_minibatch

    def spy(inds, **kw):
        before, a_before = m.critic_target.flat_params().clone(), m.actor.flat_params().clone()
        out = inner(inds, **kw)
        tau = agent.target_ema_rate
        want = before.cpu() * (1.0 - tau) + m.critic.flat_params().cpu() * tau
        polyak_ok.append(torch.equal(m.critic_target.flat_params().cpu(), want))
        actor_after[agent.itr] = m.actor.flat_params().clone()
        if agent.itr < agent.n_critic_warmup_itr:
            warm.append(bool(torch.isfinite(out[1])) and bool(m.last_loss_grad.abs().sum() > 0) and
                        torch.equal(m.actor.flat_params(), a_before))
        return out
    agent.update_minibatch = spy
    res = agent.run()
    assert [r["itr"] for r in res] == [0, 1, 2] and all(np.isfinite(r["loss_actor"]) and np.isfinite(r["loss_critic"]) for r in res)
    assert len(polyak_ok) == 3 * int(4 * 8 / 16 * 2) and all(polyak_ok)
    assert len(warm) == 4 and all(warm)
    assert torch.equal(actor_after[0], actor0) and not torch.equal(actor_after[1], actor0)
    assert not torch.equal(m.critic.flat_params(), critic0)
    data = torch.load(os.path.join(str(tmp_path), "checkpoint", "state_2.pt"), weights_only=True)
    assert {k.split(".")[0] for k in data["model"]} == {"network", "actor", "critic", "critic_target"}
    other = TrainDQLDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0))
    other.load(2)
    for a, b in ((other.model.actor, m.actor), (other.model.critic, m.critic), (other.model.critic_target, m.critic_target)):
        assert torch.equal(a.flat_params(), b.flat_params())


@pytest.mark.gpu
def test_hip_dql_agent_minibatch_is_the_recorded_sequence(golden, tmp_path):
    """One fp32 ``update_minibatch`` on the recorded rows against the sequence the reference recorded, at
    tests/test_qsm.py::test_hip_qsm_agent_minibatch_is_the_recorded_sequence's tolerances."""
    from dppo_amd.agent.finetune.train_dql_diffusion_agent import TrainDQLDiffusionAgent
    from dppo_amd.util.optim import FlatAdamW
    from dppo_amd.util.replay import DeviceReplay
    g = golden("g26_dql")
    agent = TrainDQLDiffusionAgent(agent_cfg(tmp_path, n_train_itr=0, n_critic_warmup_itr=0, target_ema_rate=K.SEQ_TAU))
    m = agent.model = make_model("hopper", "fp32", DEV)
    agent.gamma, agent.eta, agent.max_grad_norm = K.GAMMA, K.ETA, None
    agent.critic_optimizer = FlatAdamW(m.critic.flat_params(), lr=K.SEQ_LR, weight_decay=0)
    agent.actor_optimizer = FlatAdamW(m.actor.flat_params(), lr=K.SEQ_ACTOR_LR, weight_decay=0)
    b = {k: v.to(DEV) for k, v in K.critic_batch(77).items()}
    rp = agent.replay = DeviceReplay(77, 1, 11, 12, device=DEV)
    for dst, key in ((rp.obs, "obs"), (rp.next_obs, "next_obs"), (rp.actions, "actions"), (rp.reward, "reward"),
                     (rp.terminated, "terminated")):
        dst.copy_(b[key].reshape(dst.shape))
    rp.steps = 77
    lc, la = agent.update_minibatch(torch.arange(77, device=DEV), next_actions=b["next_actions"], noise=b["noise"],
                                    noise_bc=b["noise_bc"], t_bc=b["t_bc"], which=0)
    print(f"seq: critic {float(lc)!r} ref {float(g['seq_c_loss'])!r}; actor {float(la)!r} ref {float(g['seq_a_loss'])!r}")
    np.testing.assert_allclose([float(lc), float(la)], [float(g["seq_c_loss"]), float(g["seq_a_loss"])], rtol=2e-4, atol=2e-5)
    check_grads_fp32(g, "seq_gq", named_grads(m.critic, m.critic.flat_grads()))
    check_grads_fp32(g, "seq_ga", named_grads(m.actor, m.last_loss_grad))
    for key, net, gkey, step in (("seq_q", m.critic, "seq_gq", K.SEQ_LR), ("seq_actor", m.actor, "seq_ga", K.SEQ_ACTOR_LR),
                                 ("seq_target", m.critic_target, "seq_gq", K.SEQ_LR * K.SEQ_TAU)):
        check_stepped(g, key, list(net.named_parameters()), gkey, step)


# ---------------------------------------------------------------------------------------------------------------- bf16
def rel_errors(ref, got):
    """Of one run against the fp32 restatement on the same chain and masks: loss, d_a, per tensor, 1 - cosine of the whole gradient."""
    err = lambda r, x: float(np.linalg.norm(x - r) / (np.linalg.norm(r) + 1e-30))
    f = lambda t: t.detach().double().cpu().numpy().reshape(-1)
    per = {k: err(f(r), f(x)) for (k, r), (_, x) in zip(ref["named"], got["named"])}
    r, x = np.concatenate([f(v) for _, v in ref["named"]]), np.concatenate([f(v) for _, v in got["named"]])
    return dict(loss=abs(float(got["loss"]) - float(ref["loss"])) / max(1.0, abs(float(ref["loss"]))), d_a=err(f(ref["d_a"]), f(got["d_a"])),
                per=per, one_minus_cos=1.0 - float(r @ x / np.sqrt((r @ r) * (x @ x))))


def bf16_figures(g, case, n):
    """Runs the bf16 call on the given chain; returns (the yardstick's errors e_y, the call's errors, mask disagreement with the
    reference of the call and of the yardstick run with its own masks)."""
    m, chain = make_model(case, "bf16", DEV), given_chain(g, case, n)
    res = run_actor(m, case, n, chain)
    masks = res["masks"].cpu().numpy().astype(bool)
    fp32 = restate_on(case, n, chain, masks)
    yard = restate_on(case, n, chain, masks, bf16=True)
    call = dict(loss=res["loss"], d_a=res["d_a"], named=named_grads(m.actor, res["ga"]))
    own = restate_on(case, n, chain, None, bf16=True)["masks"]
    want = ref_masks(g, case, n)
    return rel_errors(fp32, yard), rel_errors(fp32, call), int((masks != want).sum()), int((own != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", K.CASES, ids=IDS)
def test_hip_dql_bf16_within_twice_the_rounding_yardstick(golden, case, n):
    e_y, e_c, mism, mism_y = bf16_figures(golden("g26_dql"), case, n)
    worst = max(e_c["per"], key=lambda k: e_c["per"][k] / (e_y["per"][k] + 1e-30))
    print(f"{case}_{n} bf16: yardstick loss {e_y['loss']:.3e} d_a {e_y['d_a']:.3e} 1-cos {e_y['one_minus_cos']:.3e}; call loss "
          f"{e_c['loss']:.3e} d_a {e_c['d_a']:.3e} 1-cos {e_c['one_minus_cos']:.3e}; worst tensor {worst}: {e_c['per'][worst]:.3e} "
          f"against {e_y['per'][worst]:.3e}; masks off {mism} (yardstick {mism_y})")
    assert e_c["loss"] <= 2 * e_y["loss"] and e_c["d_a"] <= 2 * e_y["d_a"] and e_c["one_minus_cos"] <= 2 * e_y["one_minus_cos"]
    for k in e_c["per"]:
        assert e_c["per"][k] <= 2 * e_y["per"][k], (k, e_c["per"][k], e_y["per"][k])
    assert mism <= 2 * mism_y
