"""Case table, seeded recipes and a plain-torch restatement of Cal-QL's critic loss (reference model/rl/gaussian_calql.py:56-171),
shared by make_golden_calql.py (generator, needs the reference) and tests/test_calql.py (no reference needed).

Nothing large is stored in g29_calql.npz: weights and inputs come from the seeded recipes below.  The trunks are the LayerNorm Q
trunks of make_golden_rlpd_cases.py (its ``q_forward`` on its ``q_spec``; ``bf16_linears`` / ``relu_gates`` are the contexts it
re-exports) and the actor is make_golden_sac_cases.py's (its ``sample``); a case of this file is lent to those two tables under a
``calql_`` name for the length of a call.

The restatement is written with the two scalars L = logsumexp_m(-log_pi[m]), L' = logsumexp_m(-log_pi_next[m]) in place of the
reference's (N, N) broadcast (``per_row=False``; float32 reproduces the fixture, which licenses it) or with the Cal-QL paper's
per-row -log_pi[n] (``per_row=True``), and takes a dtype: float64 fed the same fp32 values is the yardstick of the GPU tests.

``returns`` (and ``tiny_clip``'s two clip values) are CONSTRUCTED from the float64 restatement's Q values, per mode, so that every
gate is decided by construction: each of the 4 N calibration comparisons max(q, returns) and each clamp comparison of ``tiny_clip``
sits at least GUARD from its threshold."""
import functools
import math
from contextlib import contextmanager

import numpy as np
import torch

from tests.golden import make_golden_rlpd_cases as RL
from tests.golden import make_golden_sac_cases as S
from tests.golden.make_golden_rlpd_cases import RELU_TIE, VAR_FLOOR, bf16_linears, relu_gates  # noqa: F401  (re-exported)

O = RL.O
# case -> (obs_dim, Ta, Da, widths of the trunks AND of the actor's base, activation, R, S)
CALQL_NETS = {
    "tiny": (11, 1, 3, [64, 64], "ReLU", 4, 3),               # N = 1: M = 7 rows, L over one element; N = 77: M = 539 straddles 64-row blocks
    "chunk": (22, 4, 7, [128, 128, 128], "Mish", 10, 10),     # c = 0.5^28 = 2^-28
    "kitchen": (60, 1, 9, [256, 256, 256], "ReLU", 10, 10),   # gym/finetune/kitchen-*/calql_mlp_online.yaml: M = 3328
    "tiny_clip": (11, 1, 3, [64, 64], "ReLU", 4, 3),          # tiny with finite clips: rows clipped on each side
}
CASES = [("tiny", 1), ("tiny", 77), ("chunk", 77), ("kitchen", 256), ("tiny_clip", 77)]
SEED_Q, SEED_TARGET, SEED_ACTOR = 2901, 2951, 2991
Q_SCALE, TARGET_EPS = 3.0, 0.05
GAMMA, MIN_Q_WEIGHT = 0.99, 5.0
NOISE_CAP = S.NOISE_CAP
# GUARD = 8 x the largest |q - q64| of the bf16-Linear restatement (every Linear's operands rounded to bf16) over all rows, both
# trunks and all CASES, measured on the CPU by measure_guard(): 2.828e-2 (chunk_77), so GUARD = 2.262e-1.  The bf16 test allows the call twice the
# yardstick's error, so 8 leaves a factor of four.
BF16_Q_ERR = 2.828e-2
GUARD = 8 * BF16_Q_ERR
GRID = 2.0 ** -10  # constructed values are multiples of this: the same fp32 bits wherever the float64 Q values are rebuilt
CLIP_WINDOW = 16.0  # tiny_clip: clip_max - clip_min


def shapes(case):
    """(obs_dim, Ta, Da) of a case."""
    return CALQL_NETS[case][:3]


def n_samples(case):
    """(R, S) of a case."""
    return CALQL_NETS[case][5:7]


def log_rand_pi(case):
    """The value the reference subtracts from the random rows' Q: 0.5 ** (Ta * Da)."""
    _, ta, da = shapes(case)
    return 0.5 ** (ta * da)


@contextmanager
def _lent(case):
    """The case under a ``calql_`` name in RLPD_NETS and SAC_NETS, for the length of one call into those modules."""
    od, ta, da, dims, act, _, _ = CALQL_NETS[case]
    key = "calql_" + case
    RL.RLPD_NETS[key] = (od, ta, da, list(dims), act, 2)
    S.SAC_NETS[key] = (od, ta, da, list(dims), act, 1.0, 1.0)
    try:
        yield key
    finally:
        del RL.RLPD_NETS[key], S.SAC_NETS[key]


def _index(case):
    return list(CALQL_NETS).index(case.split("_")[0])  # tiny_clip shares tiny's weights


def q_spec(case):
    with _lent(case) as key:
        return RL.q_spec(key)


def twin_params(case, eps=0.0):
    """State dict of CriticObsAct(use_layernorm=True, double_q=True): Q{1,2}.moduleList.{i}.{linear_1,norm_1}.*, in the reference's
    order.  eps != 0 adds the target's perturbation."""
    spec, out = q_spec(case), {}
    for i in range(2):
        k = 100 * _index(case) + i
        p, d = O.init_params(spec, SEED_Q + k, Q_SCALE), O.init_params(spec, SEED_TARGET + k, Q_SCALE)
        for key in p:
            out[key.replace("Q1.", f"Q{i + 1}.")] = p[key] + np.float32(eps) * d[key] if eps else p[key]
    return out


def trunk(q, i):
    """Trunk i (1 or 2) of a twin's dict under the single critic's names (the same tensors: leaves stay leaves)."""
    return {k.replace(f"Q{i}.", "Q1."): v for k, v in q.items() if k.startswith(f"Q{i}.")}


def actor_params(case):
    """State dict of Gaussian_MLP(fixed_std=None, tanh_output=False), make_golden_sac_cases.actor_params's recipe on this case."""
    od, ta, da, dims, _, _, _ = CALQL_NETS[case]
    rs = np.random.RandomState(SEED_ACTOR + 10 * _index(case))
    lmin, lmax = S.logvar_bounds()
    p = {"logvar_min": lmin, "logvar_max": lmax}

    def lin(name, i, o):
        b = 1.0 / math.sqrt(i)
        p[f"{name}.weight"] = torch.from_numpy(rs.uniform(-b, b, size=(o, i)).astype(np.float32))
        p[f"{name}.bias"] = torch.from_numpy(rs.uniform(-b, b, size=(o,)).astype(np.float32))
    widths = [od] + list(dims)
    for i in range(len(widths) - 1):
        lin(f"mlp_base.moduleList.{i}.linear_1", widths[i], widths[i + 1])
    lin("mlp_mean.moduleList.0.linear_1", dims[-1], ta * da)
    lin("mlp_logvar.moduleList.0.linear_1", dims[-1], ta * da)
    return p


@functools.lru_cache(maxsize=None)
def _inputs(case, n):
    od, ta, da = shapes(case)
    R, Sn = n_samples(case)
    rs = np.random.RandomState(3000 + 17 * _index(case) + n)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    obs, nxt, act = f(n, 1, od), f(n, 1, od), f(n, ta, da)
    reward = torch.from_numpy(rs.uniform(0, 4, size=n).astype(np.float32))
    terminated = torch.from_numpy((rs.uniform(size=n) < 0.3).astype(np.float32))
    random_actions = f(n, R, ta, da)
    noise = torch.from_numpy(np.clip(rs.randn(n * (Sn + 2), ta, da), -NOISE_CAP, NOISE_CAP).astype(np.float32))
    return dict(obs=obs, next_obs=nxt, actions=act, reward=reward, terminated=terminated, random_actions=random_actions, noise=noise)


def inputs(case, n):
    """The n seeded transitions of a case, the random actions (n, R, Ta, Da) in [-1, 1) and the policy's draws ``noise`` (n (S + 2),
    Ta, Da) in the reference's call order: next x S (row n S + s), pi, pi_next.  (``returns``: returns_of.)"""
    return dict(_inputs(case, n))


@functools.lru_cache(maxsize=None)
def samples(case, n):
    """The three policy samples from the fp32 restatement of the actor on ``inputs``' draws: what every implementation is fed.
    dict(next_actions (n S, AF), pi_actions (n, AF), log_pi (n,), pi_next_actions (n, AF), log_pi_next (n,)), fp32."""
    b, (R, Sn) = _inputs(case, n), n_samples(case)
    cur, nxt = b["obs"].reshape(n, -1), b["next_obs"].reshape(n, -1)
    with _lent(case) as key, torch.no_grad():
        s = S.sample(actor_params(case), key, torch.cat([nxt.repeat_interleave(Sn, dim=0), cur, nxt]), b["noise"])
    a, lp = s["a"], s["logp"]
    return dict(next_actions=a[:n * Sn], pi_actions=a[n * Sn:n * Sn + n], log_pi=lp[n * Sn:n * Sn + n],
                pi_next_actions=a[n * Sn + n:], log_pi_next=lp[n * Sn + n:])


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def q_forward(p, case, obs, act):
    """One trunk's Q (rows,): make_golden_rlpd_cases.q_forward on this case's spec."""
    with _lent(case) as key:
        return RL.q_forward(p, key, obs, act)


def q_rows(q, case, b, sm, dtype):
    """Both trunks' Q on the four segments of the critic's rows: [(qd (n,), q_rand (n, R), q_pi (n,), q_pi_next (n,)) for i in 1, 2]."""
    n, (R, _) = len(b["obs"]), n_samples(case)
    c = lambda x: x.to(dtype)
    obs, nxt = c(b["obs"]).reshape(n, -1), c(b["next_obs"]).reshape(n, -1)
    out = []
    for i in (1, 2):
        p = trunk(q, i)
        qd = q_forward(p, case, obs, c(b["actions"]))
        qr = q_forward(p, case, obs.repeat_interleave(R, dim=0), c(b["random_actions"]).reshape(n * R, -1)).view(n, R)
        qp = q_forward(p, case, obs, c(sm["pi_actions"]))
        qn = q_forward(p, case, nxt, c(sm["pi_next_actions"]))
        out.append((qd, qr, qp, qn))
    return out


def target(tq, case, b, sm, dtype, gamma=GAMMA):
    """y (n,) = r + gamma (1 - terminated) max_s min(tq1, tq2)(next_obs_n, a'_{n,s}); also (tq1, tq2) (n S,)."""
    n, (_, Sn) = len(b["obs"]), n_samples(case)
    c = lambda x: x.to(dtype)
    with torch.no_grad():
        nxt = c(b["next_obs"]).reshape(n, -1).repeat_interleave(Sn, dim=0)
        t1, t2 = (q_forward(RL.cast(trunk(tq, i), dtype), case, nxt, c(sm["next_actions"])) for i in (1, 2))
        next_q = torch.min(t1, t2).view(n, Sn).max(dim=1).values
        return c(b["reward"]) + gamma * (1 - c(b["terminated"])) * next_q, (t1, t2)


def ood_terms(rows, sm, returns, case, per_row, dtype):
    """Per trunk (ood (n,), A (n,), A' (n,)) with the offsets of the mode."""
    lp, lpn = sm["log_pi"].to(dtype), sm["log_pi_next"].to(dtype)
    oa, ob = (-lp, -lpn) if per_row else (torch.logsumexp(-lp, 0), torch.logsumexp(-lpn, 0))
    c, out = log_rand_pi(case), []
    for qd, qr, qp, qn in rows:
        A, An = torch.max(qp, returns), torch.max(qn, returns)
        cat = torch.cat([qr - c, (A + oa)[:, None], (An + ob)[:, None]], dim=-1)
        out.append((torch.logsumexp(cat, dim=-1), A, An))
    return out


def loss_critic(q, tq, case, b, sm, returns, per_row=False, clips=(-math.inf, math.inf), w=MIN_Q_WEIGHT, gamma=GAMMA,
                dtype=torch.float32, host_stats=True):
    """gaussian_calql.py:56-171 with the policy's samples taken from ``sm``.  q: leaf tensors of ``dtype``; tq: a plain dict.
    Returns loss, stats {loss, td_1 + td_2, mean diff_1, mean diff_2, mean q1, mean y}, y, rows, diffs (unclamped, per trunk) and
    grads (in q's order).  host_stats=False leaves ``stats`` a tensor where the inputs live (tools/calql_bench.py: no read-back)."""
    returns = returns.to(dtype)
    y, tqs = target(tq, case, b, sm, dtype, gamma)
    rows = q_rows(q, case, b, sm, dtype)
    terms = ood_terms(rows, sm, returns, case, per_row, dtype)
    td = [torch.nn.functional.mse_loss(r[0], y) for r in rows]
    raw = [t[0] - r[0] for t, r in zip(terms, rows)]
    diff = [torch.clamp(x, min=clips[0], max=clips[1]).mean() for x in raw]
    loss = td[0] + td[1] + diff[0] * w + diff[1] * w
    grads = list(torch.autograd.grad(loss, list(q.values())))
    stats = torch.stack([loss, td[0] + td[1], diff[0], diff[1], rows[0][0].mean(), y.mean()]).detach()
    return dict(loss=loss.detach(), stats=[float(x) for x in stats.tolist()] if host_stats else stats,
                y=y, tq=tqs, rows=[[t.detach() for t in r] for r in rows], diffs=[x.detach() for x in raw], grads=grads)


# ---- returns and clips, by construction -----------------------------------------------------------------------------------------
def _snap_up(x):
    return math.ceil(x / GRID) * GRID


@functools.lru_cache(maxsize=None)
def _constructed(case, n, per_row):
    """(returns (n,) fp32, (clip_min, clip_max)) from the float64 restatement's Q values.  Row n's class is n % 3.
    Without clips: 0 -> returns below all four of the row's q (none binds), 1 -> above all four (all bind), 2 -> in the widest gap
    between them where it is wide enough, else as 1.  tiny_clip: class 0 keeps its natural difference and clip_min is set above all
    of those (clipped low), class 1 is lifted into the window (passes), class 2 past clip_max (clipped high); the difference of both
    trunks grows with returns, so each is found by bisection.  Every choice keeps 2 GUARD from its threshold before it is snapped."""
    D = torch.float64
    b, sm = _inputs(case, n), samples(case, n)
    with torch.no_grad():
        rows = q_rows(RL.cast(twin_params(case), D), case, b, sm, D)
    q4 = torch.stack([rows[0][2], rows[1][2], rows[0][3], rows[1][3]], dim=1).numpy()  # (n, 4)
    m = 2 * GUARD + 2 * GRID

    def clear(r, i):  # the next multiple of GRID at or above r that keeps m from all four of row i's q
        r = _snap_up(r)
        while np.abs(q4[i] - r).min() < m:
            r = _snap_up(q4[i][np.abs(q4[i] - r) < m].max() + m)
        return r

    def diffs(i, r):  # both trunks' ood - qd of row i at returns r
        ret = torch.full((n,), -1e6, dtype=D)
        ret[i] = r
        with torch.no_grad():
            t = ood_terms(rows, sm, ret, case, per_row, D)
        return np.array([float(t[k][0][i] - rows[k][0][i]) for k in range(2)])

    def lift(i, want):  # the smallest returns (cleared) at which both differences reach ``want``
        lo, hi = float(q4[i].min()) - 1.0, float(q4[i].max()) + abs(want) + 64.0
        if diffs(i, lo).min() >= want:  # already there with nothing binding
            return -_snap_up(-(float(q4[i].min()) - m - 0.25))
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if diffs(i, mid).min() >= want else (mid, hi)
        return clear(hi, i)

    ret, clips = np.zeros(n), (-math.inf, math.inf)
    if case != "tiny_clip":
        for i in range(n):
            s = np.sort(q4[i])
            k = int(np.argmax(np.diff(s)))
            if i % 3 == 0:
                ret[i] = -_snap_up(-(s[0] - m - 0.25))
            elif i % 3 == 2 and s[k + 1] - s[k] >= 2 * m + 2 * GRID:
                ret[i] = _snap_up(0.5 * (s[k] + s[k + 1]))
            else:
                ret[i] = _snap_up(s[3] + m + 0.25)
    else:
        low = [i for i in range(n) if i % 3 == 0]
        for i in low:
            ret[i] = -_snap_up(-(q4[i].min() - m - 0.25))
        lo = _snap_up(max(diffs(i, ret[i]).max() for i in low) + m)
        clips = (lo, lo + CLIP_WINDOW)
        for i in range(n):
            if i % 3 == 1:
                ret[i] = lift(i, lo + m + 0.5)
            elif i % 3 == 2:
                ret[i] = lift(i, clips[1] + m + 0.5)
    return torch.from_numpy(ret.astype(np.float32)), clips


def returns_of(case, n, per_row=False):
    """The Monte-Carlo returns (n,) of a case in a mode: constructed, see _constructed."""
    return _constructed(case, n, bool(per_row))[0].clone()


def clips_of(case, n, per_row=False):
    """(cql_clip_diff_min, cql_clip_diff_max): infinite outside ``tiny_clip``."""
    return _constructed(case, n, bool(per_row))[1]


def measure_guard():
    """The largest |q - q64| of the bf16-Linear restatement over every critic row of every case (prints it per case)."""
    worst = 0.0
    for case, n in CASES:
        b, sm = _inputs(case, n), samples(case, n)
        with torch.no_grad():
            r64 = q_rows(RL.cast(twin_params(case), torch.float64), case, b, sm, torch.float64)
            with bf16_linears():
                r16 = q_rows(twin_params(case), case, b, sm, torch.float32)
        e = max(float((x.double() - y).abs().max()) for a, c in zip(r16, r64) for x, y in zip(a, c))
        print(f"{case}_{n}: max |q_bf16 - q64| = {e:.3e}")
        worst = max(worst, e)
    print(f"largest {worst:.3e}; GUARD = 8 x = {8 * worst:.3e}")
    return worst


if __name__ == "__main__":
    measure_guard()
