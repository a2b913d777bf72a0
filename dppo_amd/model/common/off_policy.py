"""What the off-policy models share (``IDQLDiffusion``, ``QSMDiffusion``, ``DQLDiffusion`` on ``DiffusionModel``, ``SAC_Gaussian`` on
``GaussianModel``): how a minibatch reaches the library (``dppo_idql_batch`` over a ``DeviceReplay`` or over plain tensors), the
gathered observation rows, the Polyak target, the loss shim of a critic, and the sampled-bootstrap TD loss of a twin critic.
Plain functions: the models have two different bases.  ``who`` is the algorithm's name in the error texts."""
from __future__ import annotations

import ctypes as C

import torch

from dppo_amd import hip
from dppo_amd.model.diffusion.diffusion import _FusedDenoiseLoss
from dppo_amd.util.replay import DeviceReplay


def state_of(obs, who):
    if isinstance(obs, dict):
        if "rgb" in obs:
            raise NotImplementedError(f"dppo_amd: {who} is built for state observations only (like the reference)")
        obs = obs["state"]
    return obs


def as_batch(who, obs, inds=None, actions=None, next_obs=None, rewards=None, terminated=None):
    """(dppo_idql_batch, N, tensors to keep alive).  ``obs``: a ``DeviceReplay`` (rows ``inds``, or all of it) or the reference's
    ``{"state": (N, To, Do)}`` with plain (N, ...) companions (any may be missing)."""
    if isinstance(obs, DeviceReplay):
        N = len(obs) if inds is None else inds.numel()
        if inds is not None:
            assert inds.dtype == torch.int64 and inds.is_contiguous() and inds.is_cuda
        return obs.batch(inds), N, (inds,)
    st = state_of(obs, who)
    hip.require_gpu(st, who)
    N = st.shape[0]
    flat = lambda x, *s: None if x is None else x.reshape(N, *s).contiguous().float()
    keep = [flat(st, -1), None if next_obs is None else flat(state_of(next_obs, who), -1), flat(actions, -1), flat(rewards),
            flat(terminated)]
    return hip.IdqlBatch(*[hip.ptr(k) for k in keep], None, N, 1, 0, N), N, keep


def rows_of(who, obs, inds=None, nxt=False):
    """The observations (``nxt``: the next observations) of a minibatch, one row each: rows ``inds`` of a ``DeviceReplay`` in its
    logical order (one gather, not ``DeviceReplay.gather``'s five), or the plain observations themselves."""
    if isinstance(obs, DeviceReplay):
        src = obs.next_obs if nxt else obs.obs
        flat = src.reshape(obs.cap * obs.n_envs, -1)
        if inds is None and obs.head == 0:
            return flat[:len(obs)]
        return flat[obs.slot_of(torch.arange(len(obs), device=src.device) if inds is None else inds)]
    return state_of(obs, who)


def polyak(target_net, source_net, tau):
    """target <- target * (1 - tau) + source * tau over the flat [Q1 | Q2] image, then the target's kernel images are stale."""
    t, s = target_net.flat_params(), source_net.flat_params()
    hip.check(hip.load().dppo_polyak(t.data_ptr(), s.data_ptr(), float(tau), t.numel(), hip.stream()), "dppo_polyak")
    target_net.mark_updated()


def critic_loss(model, net, stats):
    """``stats[0]`` as a scalar whose ``.backward()`` hands every parameter of ``net`` its slice of ``net.flat_grads()``; ``stats``
    stays in ``model.last_stats``."""
    object.__setattr__(model, "last_stats", stats)
    return _FusedDenoiseLoss.apply(stats[0], net.grad_views(), *net.trunk_parameters())


def twin_td_loss(model, who, q, tq, obs, next_obs, actions, rewards, terminated, gamma, inds, next_actions, noise):
    """mean((q1 - y)^2) + mean((q2 - y)^2), y = r + gamma min(target q1, q2)(s', a') (1 - terminated), of the twin ``q`` against
    its target ``tq`` (``dppo_qsm_q_loss_fwd_bwd``); d loss / d [Q1 | Q2] parameters in ``q.flat_grads()``, ``model.last_stats``:
    {loss, mean q1, mean y}.  ``next_actions`` None: a' is sampled with ``model.forward`` at the gathered next observations
    (``noise`` (K+1, N, Ta, Da) replaces its draws)."""
    batch, N, keep = as_batch(who, obs, inds, actions, next_obs, rewards, terminated)
    dev = q.flat_params().device
    if next_actions is None:
        nxt = rows_of(who, obs, inds, nxt=True) if isinstance(obs, DeviceReplay) else state_of(next_obs, who)
        next_actions = model.forward({"state": nxt.reshape(N, -1)}, deterministic=False, noise=noise)
    next_actions = next_actions.reshape(N, -1).contiguous().float()
    lib, dq = hip.load(), q.net_desc()
    OD = q.cond_dim
    assert next_actions.shape[1] == dq.in_dim - OD, "next_actions must be (N, Ta, Da)"
    ws = model._ws_q.get(lib.dppo_qsm_q_loss_workspace_bytes(C.byref(dq), model.prec, OD, N), dev, "dppo_qsm_q_loss_workspace_bytes")
    k1, k2 = q.packed(model.prec)
    t1, t2 = tq.packed(model.prec)
    stats = torch.empty(hip.IDQL_STAT_COUNT, dtype=torch.float64, device=dev)
    hip.check(lib.dppo_qsm_q_loss_fwd_bwd(
        C.byref(dq), model.prec, q.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2), tq.flat_params().data_ptr(),
        t1.data_ptr(), hip.ptr(t2), C.byref(batch), OD, next_actions.data_ptr(), N, float(gamma), q.flat_grads().data_ptr(),
        stats.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()), "dppo_qsm_q_loss_fwd_bwd")
    return critic_loss(model, q, stats)
