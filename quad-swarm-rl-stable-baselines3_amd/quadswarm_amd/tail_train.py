"""The PPO update's policy tail on the split-f16 matrix cores (csrc/qs_policy_tail_train.h).

PPOTrainer.train evaluates, per minibatch and tower, the core and decoder chain, the head and (actor) the squashed
Gaussian's log-prob of the stored actions with torch autograd: a few dozen small launches per direction.  Here both
towers go from the feed_forward outputs and the stored actions to (values, log_prob) as one autograd node:

  forward   qs_policy_tail_train_x3: the rollout tail's arithmetic (values and, on the rollout's stored actions, log_prob
            are bitwise qs_policy_tail_x3's) with every chain layer's tanh output saved
  backward  qs_policy_tail_bwd_x3: per 64-row tile the head's backward and the chain's, writing dpre_l, the latents'
            gradients, per-block column maxima and per-block parts of the head's and log_std's gradients
  weights   dW_l, db_l = dpre_l^T y_{l-1} on qs_dw_x3_ld (layer 0: two column blocks against the two R-wide slices of
            the latents, row slices of stride 2R); the head's and log_std's gradients are the sums of the block parts;
            with dw="grouped" the chain's products as one qs_dw_group_x3 call instead (dw_group.py)
PPOTrainer(update_tail="x3"); tests/test_gpu_tail_train.py.
"""
import ctypes
import warnings

import torch

from . import _native as NAT
from .encoder_train import colmax_scales, dw_x3
from .policy_fused import F16_MAX, X3_SW, pack_mfma_weights_x3, tail_chain, tail_supports

ROWS = 64   # the kernels' row tile (csrc/qs_policy.h MROWS)


def torch_tail(policy, lat_actor, lat_critic, actions):
    """(values [B, 1], log_prob [B]) by the torch modules: what evaluate_actions does after the encoders."""
    from .ppo import head_linear, squashed_log_prob
    mean = head_linear(policy.action_net, policy.actor_decoder(policy.actor_core(lat_actor)))
    values = head_linear(policy.value_net, policy.critic_decoder(policy.critic_core(lat_critic)))
    return values, squashed_log_prob(mean, policy.log_std, actions)


class _Runner:
    """Buffers and launches for one policy's two towers (reused across minibatches of the same size)."""

    def __init__(self, policy, dw="calls"):
        c = policy.cfg
        self.R = c.rnn_size
        self.chains = (tail_chain(policy.actor_core, policy.actor_decoder),
                       tail_chain(policy.critic_core, policy.critic_decoder))
        self.heads = (policy.action_net, policy.value_net)
        self.log_std = policy.log_std
        self.n = len(self.chains[0])
        self.Win = self.R if self.n else 2 * self.R
        self.L = NAT.lib()
        self.towers = (NAT.QsTailTower * NAT.ATTN_MAX_TOWERS)()
        self.trains = (NAT.QsTailTrain * NAT.ATTN_MAX_TOWERS)()
        self.B = None
        self.pending = False
        self.group = None
        if dw == "grouped" and self.n:   # (no chain: nothing but the heads' part sums)
            from .dw_group import Group, plan_tail
            self.group = Group(plan_tail(policy), self.params(), self.R)

    def params(self):
        """FusedTailTrain.params()."""
        ps = []
        for ch, head in zip(self.chains, self.heads):
            for m in ch:
                ps += [m.weight, m.bias]
            ps += [head.weight, head.bias]
        return ps + [self.log_std]

    def _alloc(self, B, dev):
        R, n, Win = self.R, self.n, self.Win
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.B = B
        # the backward's blocks per tower: what the device holds at once (one block per CU at R 256, two at 128; two
        # towers per launch), at most one per row tile -- the partial results below do not grow with B
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.grid_x = max(1, min((B + ROWS - 1) // ROWS, cus * (2 if R == 128 else 1) // 2))
        self.buf = [dict(y=z(n, B, R), dpre=z(n, B, R), colmax=z(n, self.grid_x, R),
                         head_part=z(self.grid_x, h.out_features, Win + 1), mean=z(B, h.out_features),
                         log_std_part=z(self.grid_x, h.out_features)) for h in self.heads]
        for i, b in enumerate(self.buf):
            tr = self.trains[i]
            for l in range(n):
                tr.y[l], tr.dpre[l] = b["y"][l].data_ptr(), b["dpre"][l].data_ptr()
            tr.colmax = b["colmax"].data_ptr() if n else None
            tr.head_part, tr.mean, tr.log_std_part = b["head_part"].data_ptr(), b["mean"].data_ptr(), b["log_std_part"].data_ptr()
        if self.group is not None:
            named = [{f"{k}{l}": b[k][l] for k in ("y", "dpre") for l in range(n)} for b in self.buf]
            self.group.bind(named, [b["colmax"] for b in self.buf], B, 1, dev)

    def chain_weights(self):
        return [m.weight for ch in self.chains for m in ch]

    def _pack(self):
        """x3-pack both chains with this minibatch's values, the forward's operands and the backward's transposes in one
        batch per shape, and bind every weight pointer."""
        R, n = self.R, self.n
        fwd = self.chain_weights()
        bwd = []
        for ch in self.chains:
            for l, m in enumerate(ch):
                bwd += [m.weight[:, :R].t(), m.weight[:, R:].t()] if l == 0 else [m.weight.t()]
        pk = pack_mfma_weights_x3(fwd + bwd) if fwd else []
        keep, k = [], 2 * n
        for i, (ch, head) in enumerate(zip(self.chains, self.heads)):
            t, tr = self.towers[i], self.trains[i]
            for l, m in enumerate(ch):
                w, b = pk[i * n + l].contiguous(), m.bias.detach().contiguous()
                wt = torch.stack(pk[k:k + 2]).contiguous() if l == 0 else pk[k].contiguous()
                k += 2 if l == 0 else 1
                t.w_chain[l], t.b_chain[l], tr.w_chain_t[l] = w.data_ptr(), b.data_ptr(), wt.data_ptr()
                keep += [w, b, wt]
            w, b = head.weight.detach().contiguous(), head.bias.detach().contiguous()
            assert w.shape == (head.out_features, self.Win)
            t.w_head, t.b_head, t.n_out = w.data_ptr(), b.data_ptr(), head.out_features
            keep += [w, b]
        ls = self.log_std.detach().contiguous()
        self.towers[0].log_std, self.towers[1].log_std = ls.data_ptr(), None
        self.keep = keep + [ls]

    def _stream(self, dev):
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    @torch.no_grad()
    def forward(self, lat_actor, lat_critic, actions):
        B, dev = lat_actor.shape[0], lat_actor.device
        if self.B != B:
            self._alloc(B, dev)
        self._pack()
        self.lat, self.actions = (lat_actor, lat_critic), actions
        # the results into fresh tensors (autograd owns them)
        values = torch.empty(B, 1, dtype=torch.float32, device=dev)
        log_prob = torch.empty(B, dtype=torch.float32, device=dev)
        ta, tc = self.towers
        ta.x, ta.out, ta.log_prob = lat_actor.data_ptr(), None, log_prob.data_ptr()
        tc.x, tc.out, tc.log_prob = lat_critic.data_ptr(), values.data_ptr(), None
        self.trains[0].actions = actions.data_ptr()
        NAT.check(self.L.qs_policy_tail_train_x3(B, self.R, self.n, self.towers, self.trains, 2, self._stream(dev)),
                  "qs_policy_tail_train_x3")
        self.pending = True
        return values, log_prob

    @torch.no_grad()
    def backward(self, dvalues, dlogp):
        """(dlat_actor, dlat_critic, the parameter gradients in FusedTailTrain.params() order)."""
        if not self.pending:
            raise RuntimeError("FusedTailTrain: backward without a pending forward (one backward per forward: the "
                               "activations live in buffers the next forward reuses)")
        B, R, dev = self.B, self.R, self.lat[0].device
        dv = torch.zeros(B, 1, device=dev) if dvalues is None else dvalues.contiguous()
        dl = torch.zeros(B, device=dev) if dlogp is None else dlogp.contiguous()
        dlat = [torch.empty(B, 2 * R, dtype=torch.float32, device=dev) for _ in range(2)]
        self.trains[0].dlogp, self.trains[1].dvalues = dl.data_ptr(), dv.data_ptr()
        for i in range(2):
            self.trains[i].dlat = dlat[i].data_ptr()
        NAT.check(self.L.qs_policy_tail_bwd_x3(B, R, self.n, self.towers, self.trains, 2, self.grid_x, self._stream(dev)),
                  "qs_policy_tail_bwd_x3")
        grads = self.weight_grads()
        self.pending = False
        self.lat = self.actions = None
        return dlat[0], dlat[1], grads

    def weight_grads(self):
        R, n, Win = self.R, self.n, self.Win
        if self.group is not None:   # the chain's gradients from the group, the heads' and log_std's as below
            grads = self.group.run([{"lat": lat} for lat in self.lat], self.lat[0].device)
            for i in range(2):
                hp = self.buf[i]["head_part"].sum(0)
                grads[i * (2 * n + 2) + 2 * n:(i + 1) * (2 * n + 2)] = [hp[:, :Win], hp[:, Win]]
            grads[-1] = self.buf[0]["log_std_part"].sum(0)
            return grads
        grads = []
        for i in range(2):
            b, lat = self.buf[i], self.lat[i]
            # qs_colmax_reduce takes six rows of maxima per call
            gs = torch.cat([colmax_scales(b["colmax"][k:k + 6]) for k in range(0, n, 6)]) if n else None
            for l in range(n):
                G = b["dpre"][l]
                if l == 0:   # [R, 2R]: two column blocks, A the two R-wide slices of the latents (row stride 2R)
                    d0, db = dw_x3(G, lat[:, :R], gs=gs[0], sums=True)
                    dW = torch.cat((d0, dw_x3(G, lat[:, R:], gs=gs[0])), dim=1)
                else:
                    dW, db = dw_x3(G, b["y"][l - 1], gs=gs[l], sums=True)
                grads += [dW, db]
            hp = b["head_part"].sum(0)
            grads += [hp[:, :Win], hp[:, Win]]
        return grads + [self.buf[0]["log_std_part"].sum(0)]


class _TailTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, lat_actor, lat_critic, actions, *params):
        ctx.runner = runner
        return runner.forward(lat_actor, lat_critic, actions)

    @staticmethod
    def backward(ctx, dvalues, dlogp):
        da, dc, grads = ctx.runner.backward(dvalues, dlogp)
        return (None, da, dc, None) + tuple(grads)


class FusedTailTrain:
    """Both towers' core, decoder, head and the log-prob of the stored actions for the PPO update as one autograd node on
    the HIP kernels: evaluate(lat_actor, lat_critic, actions) -> (values [B, 1], log_prob [B]), the `tail` hook of
    SwarmActorCritic.evaluate_actions.  One backward per forward (the activations live in reused buffers).  dw: the chain's
    weight gradients by one launch and torch sum per product ("calls") or as one grouped launch per node ("grouped")."""

    def __init__(self, policy, dw="calls"):
        if dw not in ("calls", "grouped"):
            raise ValueError("dw must be 'calls' or 'grouped'")
        if not tail_supports(policy):
            raise ValueError("fused update tail: needs tanh core / decoder layers of width rnn_size (128 or 256), at most "
                             f"{NAT.TAIL_MAX_LAYERS} of them, and act_dim <= {NAT.TAIL_MAX_OUT}")
        self.policy = policy
        self.runner = _Runner(policy, dw)

    def params(self):
        """The parameters evaluate() returns gradients for: per tower (actor, critic) every chain layer's weight and bias,
        then the head's; then log_std."""
        return self.runner.params()

    def weights_in_range(self):
        """Every chain weight inside the split-f16 range (|w| < 65504 / 256)?  One host read."""
        mats = self.runner.chain_weights()
        if not mats:
            return True
        big = float(torch.stack([w.detach().abs().amax() for w in mats]).amax())
        ok = big < F16_MAX / X3_SW   # NaN fails too
        if not ok:
            warnings.warn(f"fused x3 update tail: max |w| = {big:.4g} >= {F16_MAX / X3_SW:.4g}, beyond the split-f16 range; "
                          "this minibatch's tail runs in torch fp32")
        return ok

    def evaluate(self, lat_actor, lat_critic, actions):
        R = self.runner.R
        assert all(x.is_cuda and x.dtype == torch.float32 for x in (lat_actor, lat_critic, actions))
        assert lat_actor.shape == lat_critic.shape == (actions.shape[0], 2 * R) and actions.dim() == 2
        if not self.weights_in_range():
            return torch_tail(self.policy, lat_actor, lat_critic, actions)
        return _TailTrainFn.apply(self.runner, lat_actor.contiguous(), lat_critic.contiguous(),
                                  actions.detach().contiguous(), *self.params())

    __call__ = evaluate
