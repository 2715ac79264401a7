"""The PPO update's multi-head attention encoder tokens on the split-f16 matrix cores (csrc/qs_policy_mha_train.h).

PPOTrainer.train evaluates QuadMultiHeadAttentionEncoder on every minibatch with autograd; its token computation --
neighbor_embed_layer and obstacle_embed_layer, the 4-head attention, fc, the residual and the LayerNorm, 18 H x H
products per token row forward and twice that backward -- is here one autograd node over both towers:

  forward   qs_mha_encoder_train_x3: the rollout kernel's tokens (bitwise) plus the saved activations (the embed layers'
            tanh outputs x1 and X, the softmax weights, the LayerNorm's normalised rows and 1 / sigma)
  backward  qs_mha_bwd_x3: LayerNorm, attention (Q, K, V recomputed from X) and embed-layer backward per 32-agent block,
            writing dpre2, dpre1 and per head the row mixes G_h[u] = sum_t s[t][u] dy_t and R_h[t] = sum_u ds[t][u] x_u;
            weight gradients on qs_dw_x3_ld (A = tanh rows): dW_n2 / dW_o2 from dpre2 and x1 (row slices), and per head
            E_h = G_h^T X, S_h = R_h^T X, from which attention_weight_grads assembles dWq, dWk, dWv, dWfc with H x H
            fp32 GEMMs; layer 0's dW = dpre1^T obs (K = 1 .. 64 + 16 columns) and the LayerNorm's two vectors in torch.
The encoder's self_embed_layer and feed_forward stay torch autograd.  tests/test_gpu_mha_train.py.
"""
import ctypes
import warnings

import torch

from . import _native as NAT
from .encoder_train import colmax_scales, dw_x3
from .policy_fused import (F16_MAX, MHA_TOWER_FIELDS, X3_SIN, mha_range_ok, mha_weight_range, pack_mha_tower, supports)

N_HEAD = 4
_TRAIN_W = ("w_fctp", "w_qtp", "w_ktp", "w_vtp", "w_n2tp", "w_o2tp")
_BUFS = ("x1", "x", "sm", "xhat", "rsig", "gmix", "rmix", "dpre2", "dpre1", "colmax")


def tower_params(enc):
    """The 14 parameters of one tower's token computation, in the order of FusedMhaTrain's gradients."""
    ne, oe, at = enc.neighbor_embed_layer, enc.obstacle_embed_layer, enc.attention_layer
    return [ne[0].weight, ne[0].bias, ne[2].weight, ne[2].bias, oe[0].weight, oe[0].bias, oe[2].weight, oe[2].bias,
            at.w_qs.weight, at.w_ks.weight, at.w_vs.weight, at.fc.weight, at.layer_norm.weight, at.layer_norm.bias]


def attention_weight_grads(E, S, w_qs, w_ks, w_vs, fc):
    """(dW_qs, dW_ks, dW_vs, dW_fc) of MultiHeadAttention from the per-head products E_h = G_h^T X and S_h = R_h^T X
    ([n_head, H, H]; G_h, R_h the backward kernel's row mixes, X the tokens as [2B, H] rows), with head h's blocks
    Wq_h = w_qs[hH:(h+1)H], Wk_h, Wv_h alike and Wfc_h = fc[:, hH:(h+1)H]:
      dWfc_h = E_h Wv_h^T,  dWv_h = Wfc_h^T E_h,  dWq_h = Wk_h S_h,  dWk_h = Wq_h S_h^T."""
    nh, H, _ = E.shape
    q, k, v = (w.view(nh, H, H) for w in (w_qs, w_ks, w_vs))
    f = fc.view(H, nh, H).transpose(0, 1)                      # [h] = fc[:, hH:(h+1)H]
    d_fc = torch.bmm(E, v.transpose(1, 2)).transpose(0, 1).reshape(H, nh * H)
    d_v = torch.bmm(f.transpose(1, 2), E).reshape(nh * H, H)
    d_q = torch.bmm(k, S).reshape(nh * H, H)
    d_k = torch.bmm(q, S.transpose(1, 2)).reshape(nh * H, H)
    return d_q, d_k, d_v, d_fc


class _Runner:
    """Buffers and launches for one policy's towers (reused across minibatches of the same size)."""

    def __init__(self, policy):
        c = policy.cfg
        self.H, self.so, self.nbw, self.od = c.rnn_size, c.self_obs_dim, c.neighbor_obs_dim * c.num_use_neighbor_obs, c.obstacle_obs_dim
        self.encs = (policy.actor_encoder, policy.critic_encoder)
        self.T = len(self.encs)
        self.L = NAT.lib()
        self.B = None
        self.towers = (NAT.QsMhaTower * NAT.ATTN_MAX_TOWERS)()
        self.trains = (NAT.QsMhaTrain * NAT.ATTN_MAX_TOWERS)()
        self.pending = False

    def _alloc(self, B, dev):
        H = self.H
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.B = B
        nblk = (B + 31) // 32                                  # the kernels' 32-agent blocks
        self.buf = [dict(x1=z(B, 2, H), x=z(B, 2, H), sm=z(B, N_HEAD, 2, 2), xhat=z(B, 2, H), rsig=z(B, 2),
                         gmix=z(N_HEAD, 2 * B, H), rmix=z(N_HEAD, 2 * B, H), dpre2=z(B, 2, H), dpre1=z(B, 2, H),
                         colmax=z(NAT.MHA_NCOLMAX, nblk, H)) for _ in range(self.T)]

    def _pack(self):
        """x3-pack both towers' weights with this minibatch's values (the forward's operands and the backward's
        transposes), bind every pointer.  ValueError outside the split-f16 ranges (FusedRolloutPolicy's rules)."""
        big, vnorm = mha_weight_range(self.encs)
        if not mha_range_ok(big, vnorm):
            raise ValueError(f"max |w| = {big:.4g} (limit {F16_MAX / 256.0:.4g}), max row |w_vs|_1 = {vnorm:.4g} "
                             f"(limit {F16_MAX / 16.0:.4g})")
        self.keep = [pack_mha_tower(enc, self.H, self.nbw, self.od, transposes=True) for enc in self.encs]
        for i, w in enumerate(self.keep):
            for name in MHA_TOWER_FIELDS:
                assert w[name].is_contiguous()
                setattr(self.towers[i], name, w[name].data_ptr())
            for name in _TRAIN_W:
                assert w[name].is_contiguous()
                setattr(self.trains[i], name, w[name].data_ptr())
            for name in _BUFS:
                setattr(self.trains[i], name, self.buf[i][name].data_ptr())

    @torch.no_grad()
    def forward(self, obs):
        B = obs.shape[0]
        if self.B != B:
            self._alloc(B, obs.device)
        self._pack()
        self.obs = obs
        # the tokens into fresh tensors (autograd owns them)
        outs = [torch.empty(B, 2 * self.H, dtype=torch.float32, device=obs.device) for _ in range(self.T)]
        for i in range(self.T):
            self.towers[i].out = outs[i].data_ptr()
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        NAT.check(self.L.qs_mha_encoder_train_x3(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], self.so, self.nbw, self.od,
                                                 B, self.H, self.towers, self.trains, self.T, st),
                  "qs_mha_encoder_train_x3")
        self.pending = True
        return outs

    @torch.no_grad()
    def backward(self, douts):
        if not self.pending:
            raise RuntimeError("FusedMhaTrain: backward without a pending forward (one backward per forward: the "
                               "activations live in buffers the next forward reuses)")
        grads = self.weight_grads(self.bwd_kernel(douts))
        self.pending = False
        self.obs = None
        return grads

    def bwd_kernel(self, douts):
        """qs_mha_bwd_x3 on both towers; returns the contiguous upstream gradients it read."""
        B, H, obs = self.B, self.H, self.obs
        d = []
        for i in range(self.T):
            g = douts[i]
            d.append(torch.zeros(B, 2 * H, device=obs.device) if g is None else g.contiguous())
            self.trains[i].dout = d[i].data_ptr()
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        NAT.check(self.L.qs_mha_bwd_x3(B, H, self.towers, self.trains, self.T, st), "qs_mha_bwd_x3")
        return d

    def weight_grads(self, d):
        """The 28 parameter gradients from what the backward kernel wrote."""
        B, H, so, nbw, od, obs = self.B, self.H, self.so, self.nbw, self.od, self.obs
        nbr, obst = obs[:, so:so + nbw], obs[:, so + nbw:so + nbw + od]
        grads = []
        for i, enc in enumerate(self.encs):
            b, at = self.buf[i], enc.attention_layer
            gs = torch.cat((colmax_scales(b["colmax"][:6]), colmax_scales(b["colmax"][6:])))   # [12, H] column scales
            dp2, dp1, x1 = b["dpre2"], b["dpre1"], b["x1"]
            X = b["x"].view(2 * B, H)
            # the embed layers' second Linears: a token's rows are slices of the [B, 2, H] arrays (row stride 2H)
            dw_n2, db_n2 = dw_x3(dp2[:, 0], x1[:, 0], gs=gs[0], sums=True)
            dw_o2, db_o2 = dw_x3(dp2[:, 1], x1[:, 1], gs=gs[1], sums=True)
            # their first Linears on the raw observations (64 + 16 columns: no kernel for that shape), torch
            dw_n1, db_n1 = dp1[:, 0].t().mm(nbr), dp1[:, 0].sum(0)
            dw_o1, db_o1 = dp1[:, 1].t().mm(obst), dp1[:, 1].sum(0)
            E = torch.stack([dw_x3(b["gmix"][h], X, gs=gs[4 + 2 * h]) for h in range(N_HEAD)])
            S = torch.stack([dw_x3(b["rmix"][h], X, gs=gs[5 + 2 * h]) for h in range(N_HEAD)])
            d_q, d_k, d_v, d_fc = attention_weight_grads(E, S, at.w_qs.weight.detach(), at.w_ks.weight.detach(),
                                                         at.w_vs.weight.detach(), at.fc.weight.detach())
            dout = d[i].view(2 * B, H)
            grads += [dw_n1, db_n1, dw_n2, db_n2, dw_o1, db_o1, dw_o2, db_o2, d_q, d_k, d_v, d_fc,
                      (dout * b["xhat"].view(2 * B, H)).sum(0), dout.sum(0)]
        return grads


class _MhaTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, obs, *params):
        ctx.runner = runner
        return tuple(runner.forward(obs))

    @staticmethod
    def backward(ctx, *douts):
        return (None, None) + tuple(ctx.runner.backward(douts))


class FusedMhaTrain:
    """Both towers' attention tokens for the PPO update as one autograd node on the HIP kernels: tokens(obs) ->
    [actor [B, 2H], critic [B, 2H]] (SwarmActorCritic.evaluate_actions(obs, actions, nbr=...)).  One backward per forward
    (the activations live in reused buffers)."""

    def __init__(self, policy):
        if policy.cfg.encoder_type != "attention" or not supports(policy):
            raise ValueError("fused multi-head attention update: needs encoder_type 'attention' with tanh, rnn_size 128 or "
                             "256, a neighbour block of at most 64 and at most 16 obstacle values")
        self.policy = policy
        self.runner = _Runner(policy)

    def params(self):
        return [p for enc in self.runner.encs for p in tower_params(enc)]

    def obs_in_range(self, obs):
        """True when every value of `obs` is inside the split-f16 range of layer 0 (|obs| < 4094), as
        FusedAttentionTrain.obs_in_range: beyond it the update's tokens run on torch autograd.  One host sync."""
        v = float(obs.abs().amax())
        ok = not (v == v and v != float("inf") and v * X3_SIN >= F16_MAX)
        if not ok:
            self._warn(f"an observation reached |obs| = {v:.4g} >= {F16_MAX / X3_SIN:.4g}")
        return ok

    def _warn(self, why):
        warnings.warn(f"fused x3 update: {why}, beyond the split-f16 range; this minibatch's attention tokens run in "
                      "torch fp32")

    def tokens(self, obs):
        """Both towers' tokens, or None (the caller's torch autograd path) when a weight left the split-f16 range (the
        packer refuses it before any kernel runs), as FusedAttentionTrain.encodings."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2
        try:
            return list(_MhaTrainFn.apply(self.runner, obs.contiguous(), *self.params()))
        except ValueError as e:
            self._warn(str(e))
            return None
