"""The PPO update's MLP-family encoders on the split-f16 matrix cores (csrc/qs_policy_enc_train.h).

For a QuadMultiEncoder whose neighbour encoder is mlp, mean_embed or none (policy_fused.encoder_supports), PPOTrainer.train
runs both towers' encoders through torch for every minibatch: two to four small branches per tower, a cat, the
feed_forward, and their autograd.  Here both towers go from the minibatch's raw observations to the feed_forward outputs
[B, 2H] as one autograd node:

  forward   qs_encoder_mlp_train_x3: the rollout kernel's arithmetic (out is bitwise qs_encoder_mlp_x3's) with every tanh
            layer's output saved
  backward  qs_encoder_mlp_bwd_x3: per 64-agent tile the feed_forward's backward and every branch's chain, writing the
            pre-activation gradients and per-block column maxima
  weights   dW = dpre^T (the previous layer's save) on qs_dw_x3_ld -- the [2H, NP H] feed_forward weight as its 2 NP blocks
            from column slices of dpre_ff; the self encoder's layer 0 on qs_attn_dw0_x3; the neighbour and obstacle layer 0
            from qs_colstats's part_x (at most 32 columns a call: the mlp block of up to 64 takes two); with dw="grouped"
            every product of the node as one qs_dw_group_x3 call instead (dw_group.py: the column scales, the sums over
            row parts and the block placement inside the kernels)
PPOTrainer(update_encoder="x3"); tests/test_gpu_enc_mlp_train.py.
"""
import ctypes
import warnings

import torch

from . import _native as NAT
from .encoder_train import col_stats, colmax_scales, dw0_x3, dw_x3
from .policy_fused import F16_MAX, X3_SIN, enc_nbr_kind, encoder_supports, pack_enc_towers, pack_mfma_weights_x3

ROWS = 64   # the kernels' row tile (csrc/qs_policy.h MROWS)
# qs_enc_train.colmax rows
CM_FF, CM_S1, CM_S2, CM_N1, CM_N2, CM_N3, CM_O1, CM_O2 = 0, 2, 3, 4, 5, 6, 7, 8


def branch_layers(enc):
    """One tower's Linear layers by branch: (self [2], neighbour [0, 2 or 3], obstacle [0 or 2], feed_forward)."""
    lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]  # noqa: E731
    kind = enc_nbr_kind(enc.cfg)
    nbr = [] if kind == "none" else lin(enc.neighbor_encoder.neighbor_mlp if kind == "mlp"
                                        else enc.neighbor_encoder.embedding_mlp)
    obst = lin(enc.obstacle_encoder) if enc.obstacle_encoder is not None else []
    return lin(enc.self_encoder), nbr, obst, enc.feed_forward[0]


def tower_params(enc):
    """The parameters the node returns gradients for, per tower: every self, neighbour and obstacle layer's weight and
    bias, then the feed_forward's -- 6 (none), 10 (mean), 12 (mlp), plus 4 with obstacles."""
    s, n, o, ff = branch_layers(enc)
    return [p for m in s + n + o + [ff] for p in (m.weight, m.bias)]


def ff_transposes(enc):
    """The backward's dP operands: per part p present (self, neighbour, obstacle) the [H, 2H] transpose of
    feed_forward[0].weight[:, pH:(p+1)H], to be packed like any weight."""
    H, w = enc.cfg.rnn_size, enc.feed_forward[0].weight
    return [w[:, p * H:(p + 1) * H].t() for p in range(w.shape[1] // H)]


def pack_ff_transposes(enc):
    """qs_enc_train.w_fft: ff_transposes packed, contiguous in part order ([NP, H / 32, 2H / 16, 64, 2, 8] int16)."""
    return torch.stack(pack_mfma_weights_x3(ff_transposes(enc))).contiguous()


class _Runner:
    """Buffers and launches for one policy's two towers (reused across minibatches of the same size)."""

    def __init__(self, policy, grid_x=None, dw="calls"):
        c = policy.cfg
        self.H, self.K, self.nd, self.so, self.od = (c.rnn_size, c.num_use_neighbor_obs, c.neighbor_obs_dim, c.self_obs_dim,
                                                     c.obstacle_obs_dim)
        self.kind = enc_nbr_kind(c)
        self.encs = (policy.actor_encoder, policy.critic_encoder)
        self.grid_cap = grid_x
        self.L = NAT.lib()
        self.towers = (NAT.QsEncTower * NAT.ATTN_MAX_TOWERS)()
        self.trains = (NAT.QsEncTrain * NAT.ATTN_MAX_TOWERS)()
        self.B = None
        self.pending = False
        self.group = None
        if dw == "grouped":
            from .dw_group import Group, plan_encoder
            self.group = Group(plan_encoder(policy), [p for enc in self.encs for p in tower_params(enc)], self.H)

    def _alloc(self, B, dev):
        H, K = self.H, self.K
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.B = B
        # the backward's blocks per tower: what the device holds at once (one block per CU at H 256, two at 128; two
        # towers per launch), at most one per row tile
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.grid_x = max(1, min((B + ROWS - 1) // ROWS, self.grid_cap or cus * (2 if H == 128 else 1) // 2))
        rows = dict(s1=B, s2=B)
        if self.kind == "mlp":
            rows.update(n1=B, n2=B, n3=B)
        elif self.kind == "mean":   # e1, e2 per (agent, neighbour): 2 towers x 2 layers x B K H floats, and their gradients
            rows.update(n1=B * K, n2=B * K)
        if self.od:
            rows.update(o1=B, o2=B)
        self.buf = []
        for i in range(2):
            b = {n: z(r, H) for n, r in rows.items()}
            b.update({"dpre_" + n: z(r, H) for n, r in rows.items()})
            b.update(dpre_ff=z(B, 2 * H), colmax=z(NAT.ENC_NCOLMAX, self.grid_x, H))
            if self.kind == "mean":
                b.update(m=z(B, H), dm=z(B, H))
            for n, t in b.items():
                setattr(self.trains[i], n, t.data_ptr())
            self.buf.append(b)
        if self.group is not None:
            self.group.bind(self.buf, [b["colmax"] for b in self.buf], B, K, dev)

    def _pack(self):
        """x3-pack both towers with this minibatch's values (the optimiser changed them): the forward's operands
        (pack_enc_towers; ValueError beyond the split-f16 range) and the backward's transposes, and bind the pointers."""
        fwd = pack_enc_towers(self.encs)
        mats, spans = [], []
        for enc in self.encs:
            s, n, o, _ = branch_layers(enc)
            named = [("w_s2t", s[1])] + [(f"w_n{l + 1}t", m) for l, m in enumerate(n) if l] + ([("w_o2t", o[1])] if o else [])
            spans.append(([nm for nm, _ in named], len(mats)))
            mats += [m.weight.t() for _, m in named] + ff_transposes(enc)
        pk = pack_mfma_weights_x3(mats)
        self.keep = []
        for i, (names, a) in enumerate(spans):
            t, tr = self.towers[i], self.trains[i]
            for name, x in fwd[i].items():
                assert x.is_contiguous()
                setattr(t, name, x.data_ptr())
            k = {nm: pk[a + j].contiguous() for j, nm in enumerate(names)}
            end = spans[i + 1][1] if i + 1 < len(spans) else len(pk)
            k["w_fft"] = torch.stack(pk[a + len(names):end]).contiguous()
            for nm, x in k.items():
                setattr(tr, nm, x.data_ptr())
            self.keep += [fwd[i], k]

    def _args(self, obs):
        return (ctypes.c_void_p(obs.data_ptr()), obs.shape[1], self.so, NAT.ENC_NBR[self.kind], self.K, self.nd, self.od,
                self.B, self.H, self.towers, self.trains, 2)

    def _stream(self, dev):
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    @torch.no_grad()
    def forward(self, obs):
        B, dev = obs.shape[0], obs.device
        self._pack()   # (first: a weight out of range raises before anything is allocated or launched)
        if self.B != B:
            self._alloc(B, dev)
        self.obs = obs
        # the results into fresh tensors (autograd owns them)
        self.out = [torch.empty(B, 2 * self.H, dtype=torch.float32, device=dev) for _ in range(2)]
        for i in range(2):
            self.towers[i].out = self.out[i].data_ptr()
        NAT.check(self.L.qs_encoder_mlp_train_x3(*self._args(obs), self._stream(dev)), "qs_encoder_mlp_train_x3")
        self.pending = True
        return self.out

    @torch.no_grad()
    def backward(self, douts):
        """The parameter gradients in FusedEncoderTrain.params() order."""
        if not self.pending:
            raise RuntimeError("FusedEncoderTrain: backward without a pending forward (one backward per forward: the "
                               "activations live in buffers the next forward reuses)")
        obs, dev = self.obs, self.obs.device
        d = [torch.zeros_like(o) if g is None else g.contiguous() for g, o in zip(douts, self.out)]
        for i in range(2):
            self.trains[i].dout = d[i].data_ptr()
        NAT.check(self.L.qs_encoder_mlp_bwd_x3(*self._args(obs), self.grid_x, self._stream(dev)), "qs_encoder_mlp_bwd_x3")
        if self.group is not None:
            grads = self.group.run([{"obs": obs}] * 2, dev)
        else:
            grads = [g for i in range(2) for g in self.weight_grads(self.buf[i], obs)]
        self.pending = False
        self.obs = self.out = None
        return grads

    def layer0(self, G, obs, K, off, width):
        """(dW [H, width], db) of a neighbour or obstacle layer 0 from qs_colstats's part_x: G's row r = q K + k against
        obs[q, off + k (width / ...) ..]; at most 32 columns a call."""
        B, cols, db = obs.shape[0], [], None
        per = width if K == 1 else self.nd   # K > 1: one neighbour's nd <= 16 columns per row
        for c0 in range(0, per, 32):
            w = min(32, per - c0)
            _, sums, px = col_stats(G, obs, B=B, K=K, nbr_off=off + c0, nd=w, nx=w)
            cols.append(px.t())
            db = sums if db is None else db
        return torch.cat(cols, dim=1) if len(cols) > 1 else cols[0], db

    def weight_grads(self, b, obs):
        H, K, nd, so, od, B = self.H, self.K, self.nd, self.so, self.od, self.B
        gs = torch.cat([colmax_scales(b["colmax"][:6]), colmax_scales(b["colmax"][6:])])   # six rows of maxima per call
        grads = [*dw0_x3(b["dpre_s1"], obs, B, 1, so, 0, gs=gs[CM_S1]), *dw_x3(b["dpre_s2"], b["s1"], gs=gs[CM_S2], sums=True)]
        parts = [b["s2"]]
        if self.kind == "mlp":
            grads += [*self.layer0(b["dpre_n1"], obs, 1, so, K * nd), *dw_x3(b["dpre_n2"], b["n1"], gs=gs[CM_N2], sums=True),
                      *dw_x3(b["dpre_n3"], b["n2"], gs=gs[CM_N3], sums=True)]
            parts.append(b["n3"])
        elif self.kind == "mean":
            grads += [*self.layer0(b["dpre_n1"], obs, K, so, nd), *dw_x3(b["dpre_n2"], b["n1"], gs=gs[CM_N2], sums=True)]
            parts.append(b["m"])
        if od:
            grads += [*self.layer0(b["dpre_o1"], obs, 1, so + K * nd, od), *dw_x3(b["dpre_o2"], b["o1"], gs=gs[CM_O2], sums=True)]
            parts.append(b["o2"])
        # the [2H, NP H] feed_forward weight as its 2 NP blocks: column slices of dpre_ff (row stride 2H) against the parts
        G = b["dpre_ff"]
        dW = torch.empty(2 * H, len(parts) * H, dtype=torch.float32, device=G.device)
        db = torch.empty(2 * H, dtype=torch.float32, device=G.device)
        for z in range(2):
            Gz = G[:, z * H:(z + 1) * H]
            for p, A in enumerate(parts):
                r = dw_x3(Gz, A, gs=gs[CM_FF + z], sums=p == 0)
                dW[z * H:(z + 1) * H, p * H:(p + 1) * H] = r[0] if p == 0 else r
                if p == 0:
                    db[z * H:(z + 1) * H] = r[1]
        return grads + [dW, db]


class _EncTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, obs, *params):
        ctx.runner = runner
        return tuple(runner.forward(obs))

    @staticmethod
    def backward(ctx, *douts):
        return (None, None) + tuple(ctx.runner.backward(douts))


class FusedEncoderTrain:
    """Both towers' encoders for the PPO update as one autograd node on the HIP kernels: latents(obs) -> (actor [B, 2H],
    critic [B, 2H]), the `lat` of SwarmActorCritic.evaluate_actions.  One backward per forward (the activations live in
    reused buffers).  grid_x: a cap on the backward's blocks per tower (default: from the CU count).  dw: the weight
    gradients by one launch and torch sum per product ("calls") or as one grouped launch per node ("grouped")."""

    def __init__(self, policy, grid_x=None, dw="calls"):
        if dw not in ("calls", "grouped"):
            raise ValueError("dw must be 'calls' or 'grouped'")
        if not encoder_supports(policy):
            raise ValueError("fused update encoder: needs a tanh QuadMultiEncoder with the mlp, mean_embed or no neighbour "
                             "encoder, every branch rnn_size (128 or 256) wide (policy_fused.encoder_supports)")
        self.policy = policy
        self.runner = _Runner(policy, grid_x, dw)

    def params(self):
        return [p for enc in self.runner.encs for p in tower_params(enc)]

    def obs_in_range(self, obs):
        """True when every value of `obs` (the whole rollout storage, once per update) is inside the split-f16 range of
        layer 0 (|obs| < 4094); beyond it that update's encoders run on the torch autograd path.  One host sync."""
        v = float(obs.abs().amax())
        ok = not (v == v and v != float("inf") and v * X3_SIN >= F16_MAX)
        if not ok:
            warnings.warn(f"fused x3 update encoder: an observation reached |obs| = {v:.4g} >= {F16_MAX / X3_SIN:.4g}, "
                          "beyond the split-f16 range; this update's encoders run in torch fp32")
        return ok

    def latents(self, obs):
        """(actor, critic) encoder outputs, or None (the caller's torch path) when a packed weight left the split-f16
        range (|w| >= 255.9: the packer refuses it before any kernel runs)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2
        try:
            return _EncTrainFn.apply(self.runner, obs.contiguous(), *self.params())
        except ValueError as e:
            warnings.warn(f"fused x3 update encoder: {e}; this minibatch's encoders run in torch fp32")
            return None
