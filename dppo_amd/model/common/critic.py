"""State-value critic and state-action twin critic.  Mirrors ``dppo/model/common/critic.py:15-113`` (reference ``CriticObs``,
``CriticObsAct``)."""
from __future__ import annotations

import ctypes as C
from typing import Union

import torch

from dppo_amd import hip
from dppo_amd.model.common.mlp import MLP, HipNet, ResidualMLP
from dppo_amd.model.common.vit import VisionMixin


class CriticObs(HipNet):
    """V(s) = ResidualMLP([To*Do] + mlp_dims + [1]) on the flattened observation history."""

    def __init__(self, cond_dim, mlp_dims, activation_type="Mish", use_layernorm=False, residual_style=False,
                 precision="bf16", **kwargs):
        super().__init__()
        if use_layernorm and not residual_style:
            raise NotImplementedError("dppo_amd: plain MLP with LayerNorm is built for CriticObsAct(double_q=False) only")
        self.Q1 = (ResidualMLP if residual_style else MLP)([cond_dim] + list(mlp_dims) + [1], activation_type=activation_type,
                                                           out_activation_type="Identity", use_layernorm=use_layernorm)
        self.cond_dim = cond_dim
        self.prec = hip.PREC_BY_NAME[precision]
        object.__setattr__(self, "_ws", hip.Workspace())

    def net_desc(self) -> hip.NetDesc:
        d = self.__dict__.get("_desc_cache")  # architecture is fixed after construction
        if d is None:
            q = self.Q1
            d = hip.NetDesc(kind=1, in_dim=self.cond_dim, hidden=q.hidden, n_blocks=q.n_blocks, out_dim=1, act=q.act,
                            time_dim=0, act_flat=0, cond_dim=self.cond_dim, cond_hidden=0, cond_out=0,
                            use_layernorm=q.use_layernorm, plain=q.plain)
            object.__setattr__(self, "_desc_cache", d)
        return d

    @torch.no_grad()
    def forward(self, cond: Union[dict, torch.Tensor]) -> torch.Tensor:
        """cond: {"state": (B,To,Do)} or (B, To*Do) -> (B,1).  Inference only; the training forward/backward of
        the critic lives inside PPODiffusion.loss (fused)."""
        state = cond["state"] if isinstance(cond, dict) else cond
        hip.require_gpu(state, "CriticObs.forward")
        B = state.shape[0]
        state = state.reshape(B, -1).contiguous().float()
        lib, d = hip.load(), self.net_desc()
        flat, pk = self.flat_params(), self.packed(self.prec, 0)
        out = torch.empty(B, dtype=torch.float32, device=state.device)
        wsb = lib.dppo_mlp_forward_workspace_bytes(C.byref(d), self.prec, B)
        ws = self._ws.get(wsb, state.device)
        hip.check(lib.dppo_critic_forward(C.byref(d), self.prec, flat.data_ptr(), pk.data_ptr(), state.data_ptr(), B,
                                          out.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream()),
                  "dppo_critic_forward")
        return out.view(B, 1)


class _QTrunk(HipNet):
    """One Q trunk as the library sees it: a kind-1 network on the [obs | action] row whose flat buffer is a slice of the
    owner's."""

    def __init__(self, module, in_dim):
        super().__init__()
        object.__setattr__(self, "_m", module)
        self.in_dim = in_dim

    def trunk_parameters(self):
        return list(self._m.parameters())

    def net_desc(self) -> hip.NetDesc:
        d = self.__dict__.get("_desc_cache")
        if d is None:
            m = self._m
            d = hip.NetDesc(kind=1, in_dim=self.in_dim, hidden=m.hidden, n_blocks=m.n_blocks, out_dim=1, act=m.act, time_dim=0,
                            act_flat=0, cond_dim=self.in_dim, cond_hidden=0, cond_out=0, use_layernorm=m.use_layernorm,
                            plain=m.plain)
            object.__setattr__(self, "_desc_cache", d)
        return d


class CriticObsAct(HipNet):
    """Q1(s, a), Q2(s, a) on cat[To*Do observation history, Ta*Da action chunk].  The keyword that selects the residual trunk is
    spelled ``residual_tyle`` in the reference and ``**kwargs`` swallows every other spelling: the shipped cfgs pass
    ``residual_style: True`` and therefore build PLAIN trunks (``Q{1,2}.moduleList.{i}.linear_1.*``).  Kept, typo included, so
    that reference checkpoints load.  The two trunks sit back to back in ONE flat fp32 buffer [Q1 | Q2]."""

    is_composite = True  # two kernel images

    def __init__(self, cond_dim, mlp_dims, action_dim, action_steps=1, activation_type="Mish", use_layernorm=False,
                 residual_tyle=False, double_q=True, precision="bf16", twin_layernorm=False, **kwargs):
        super().__init__()
        self.cond_dim, self.act_flat = cond_dim, action_dim * action_steps
        dims = [cond_dim + self.act_flat] + list(mlp_dims) + [1]
        model = ResidualMLP if residual_tyle else MLP
        # A twin of LayerNorm trunks is read by Cal-QL's critic loss alone (csrc/calql.h): every other twin entry of the library
        # refuses a LayerNorm descriptor, so the combination is opt-in (``twin_layernorm=True``; CalQL_Gaussian's cfg node asks for it)
        if use_layernorm and not residual_tyle and double_q and not twin_layernorm:
            raise NotImplementedError("dppo_amd: plain MLP with LayerNorm is built for CriticObsAct(double_q=False), and as a twin "
                                      "for Cal-QL only (twin_layernorm=True)")
        self.twin_layernorm = bool(twin_layernorm and use_layernorm and not residual_tyle and double_q)
        self.Q1 = model(dims, activation_type=activation_type, out_activation_type="Identity", use_layernorm=use_layernorm)
        if double_q:
            self.Q2 = model(dims, activation_type=activation_type, out_activation_type="Identity", use_layernorm=use_layernorm)
        self.double_q = bool(double_q)
        self.prec = hip.PREC_BY_NAME[precision]
        object.__setattr__(self, "_ws", hip.Workspace())

    def __deepcopy__(self, memo):
        new = HipNet.__deepcopy__(self, memo)  # parameters copied, flat image / kernel images / trunk views rebuilt on use
        new.__dict__.pop("_trunk_nets", None)
        object.__setattr__(new, "_ws", hip.Workspace())
        return new

    def trunk_parameters(self):
        return list(self.Q1.parameters()) + (list(self.Q2.parameters()) if self.double_q else [])

    def _abi_param_count(self) -> int:
        return hip.load().dppo_net_param_count(C.byref(self.net_desc())) * (2 if self.double_q else 1)

    def net_desc(self) -> hip.NetDesc:
        """The descriptor both trunks share."""
        return self._trunks(bind=False)[0].net_desc()

    def _trunks(self, bind=True):
        t = self.__dict__.get("_trunk_nets")
        if t is None:
            n_in = self.cond_dim + self.act_flat
            t = (_QTrunk(self.Q1, n_in),) + ((_QTrunk(self.Q2, n_in),) if self.double_q else ())
            object.__setattr__(self, "_trunk_nets", t)
        if bind:  # (re-)attach the slices: after .to(device) / a re-homed flat buffer
            flat, grads = self.flat_params(), self.flat_grads()
            n0 = flat.numel() // len(t)
            for i, net in enumerate(t):
                lo = i * n0
                if (net._flat is None or net._flat.data_ptr() != flat.data_ptr() + 4 * lo or
                        net._flat_grad.data_ptr() != grads.data_ptr() + 4 * lo):
                    object.__setattr__(net, "_flat", flat[lo:lo + n0])
                    object.__setattr__(net, "_flat_grad", grads[lo:lo + n0])
                    net._packed.clear()
        return t

    def packed(self, prec: int, n_time: int = 0):
        """(Q1 image, Q2 image or None), re-packed when the parameters changed."""
        t = self._trunks()
        return t[0].packed(prec, 0), (t[1].packed(prec, 0) if self.double_q else None)

    def mark_updated(self):
        HipNet.mark_updated(self)
        for t in self._trunks(bind=False):
            t.mark_updated()

    @torch.no_grad()
    def forward(self, cond: Union[dict, torch.Tensor], action: torch.Tensor, obs_repeat: int = 1):
        """cond: {"state": (B,To,Do)} or (B, To*Do); action (N,Ta,Da) with N = B * obs_repeat, row n scored against
        observation n % B -> (q1 (N,), q2 (N,)), or q1 alone without a second trunk.  Inference only; the training
        forward / backward lives inside IDQLDiffusion.loss_critic_q."""
        state = cond["state"] if isinstance(cond, dict) else cond
        hip.require_gpu(state, "CriticObsAct.forward")
        B = state.shape[0]
        N = action.shape[0]
        assert N == B * obs_repeat, "action rows must be observation rows * obs_repeat"
        state = state.reshape(B, -1).contiguous().float()
        action = action.reshape(N, -1).contiguous().float()
        lib, d = hip.load(), self.net_desc()
        k1, k2 = self.packed(self.prec)
        q1 = torch.empty(N, dtype=torch.float32, device=state.device)
        q2 = torch.empty(N, dtype=torch.float32, device=state.device) if self.double_q else None
        if self.twin_layernorm:  # one trunk per call: the double_q = 1 query refuses a LayerNorm descriptor
            wsb = lib.dppo_idql_q_forward_workspace_bytes(C.byref(d), self.prec, N, 0)
            ws, flat = self._ws.get(wsb, state.device, "dppo_idql_q_forward_workspace_bytes"), self.flat_params()
            P = flat.numel() // 2
            for i, (k, out) in enumerate(((k1, q1), (k2, q2))):
                hip.check(lib.dppo_idql_q_forward(C.byref(d), self.prec, flat.data_ptr() + 4 * i * P, k.data_ptr(), None,
                                                  state.data_ptr(), state.shape[1], B, action.data_ptr(), N, 0, out.data_ptr(), None,
                                                  ws.data_ptr(), ws.numel(), hip.stream()), "dppo_idql_q_forward")
            return q1, q2
        wsb = lib.dppo_idql_q_forward_workspace_bytes(C.byref(d), self.prec, N, int(self.double_q))
        if wsb < 0:
            hip.check(int(wsb), "dppo_idql_q_forward_workspace_bytes")
        ws = self._ws.get(wsb, state.device)
        hip.check(lib.dppo_idql_q_forward(C.byref(d), self.prec, self.flat_params().data_ptr(), k1.data_ptr(), hip.ptr(k2),
                                          state.data_ptr(), state.shape[1], B, action.data_ptr(), N, int(self.double_q),
                                          q1.data_ptr(), hip.ptr(q2), ws.data_ptr(), ws.numel(), hip.stream()),
                  "dppo_idql_q_forward")
        return (q1, q2) if self.double_q else q1


class ViTCritic(VisionMixin, CriticObs):
    """ViT backbone + SpatialEmb, then the state-value MLP on cat[feat, state].  Mirrors
    ``dppo/model/common/critic.py:116-206`` (Q1 is registered before the backbone there too)."""

    def __init__(self, backbone, cond_dim, img_cond_steps=1, spatial_emb=128, dropout=0, augment=False, num_img=1,
                 precision="bf16", **kwargs):
        CriticObs.__init__(self, cond_dim=spatial_emb * num_img + cond_dim, precision=precision, **kwargs)
        self._init_vision(backbone, cond_dim, img_cond_steps, spatial_emb, num_img, augment, dropout, precision)

    def trunk_parameters(self):
        return list(self.Q1.parameters())

    @torch.no_grad()
    def forward(self, cond, no_augment=False):
        return CriticObs.forward(self, self.encode_obs(cond, augment=self.augment and not no_augment))
