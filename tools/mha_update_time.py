#!/usr/bin/env python
"""HIP-event times of the PPO update's fused multi-head attention tokens (csrc/qs_policy_mha_train.h, mha_train.py) next
to torch autograd of the module's tokens on the same inputs in the same process.

    python tools/mha_update_time.py [--B 32768] [--H 256] [--nd 6] [--K 6] [--iters 10] [--rounds 3]

mha_time.py's method: per round, alternating windows of `iters` back-to-back calls between two events, after warm-up.
fused: forward + backward producing all 28 gradients; torch: tokens + autograd.grad.  The fused side's parts are timed
in windows of their own: the forward kernel, the backward kernel, the host's gradient assembly (the qs_dw_x3_ld calls
and the torch remainder) and of that the torch-only part (layer 0's dW, the LayerNorm vectors).  FLOP per agent and
tower: forward 2 (34 H^2 + 160 H); backward kernel 116 H^2 (7 H x H layers per head and one per embed tower, two rows)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))

import torch  # noqa: E402

from mha_time import F16_PEAK, window  # noqa: E402
from quadswarm_amd.mha_train import FusedMhaTrain  # noqa: E402
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 32768), ("H", 256), ("nd", 6), ("K", 6), ("iters", 10), ("rounds", 3)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    torch.manual_seed(0)
    pc = PolicyConfig(self_obs_dim=19, neighbor_obs_dim=a.nd, num_use_neighbor_obs=a.K, obstacle_obs_dim=9, rnn_size=a.H,
                      neighbor_hidden_size=a.H, act_dim=4, encoder_type="attention")
    pol = SwarmActorCritic(pc).cuda()
    B, H = a.B, a.H
    obs = torch.randn(B, 19 + a.nd * a.K + 9, device="cuda")
    dout = torch.randn(2, B, 2 * H, device="cuda") * 1e-3
    fm = FusedMhaTrain(pol)
    params, run = fm.params(), fm.runner
    encs = (pol.actor_encoder, pol.critic_encoder)
    fused = lambda: torch.autograd.grad((torch.stack(fm.tokens(obs)) * dout).sum(), params)  # noqa: E731
    module = lambda: torch.autograd.grad((torch.stack([e.tokens(obs) for e in encs]) * dout).sum(), params)  # noqa: E731
    gf, gt = fused(), module()
    rel = max(((f - t).abs().max() / t.abs().max()).item() for f, t in zip(gf, gt))
    for _ in range(3):
        fused()
        module()
    run.forward(obs)   # the parts below reuse this forward's activations
    d = [dout[0], dout[1]]
    so, nbw = pc.self_obs_dim, a.nd * a.K

    def torch_part():
        for i in range(2):
            dp1, g = run.buf[i]["dpre1"], dout[i].view(2 * B, H)
            dp1[:, 0].t().mm(obs[:, so:so + nbw]), dp1[:, 0].sum(0), dp1[:, 1].t().mm(obs[:, so + nbw:]), dp1[:, 1].sum(0)
            (g * run.buf[i]["xhat"].view(2 * B, H)).sum(0), g.sum(0)

    with torch.no_grad():
        run.bwd_kernel(d)
        t = dict(fused_ms=[], torch_ms=[], fwd_kernel_ms=[], bwd_kernel_ms=[], assembly_ms=[], assembly_torch_only_ms=[])
        for _ in range(a.rounds):
            with torch.enable_grad():
                t["fused_ms"].append(window(fused, a.iters))
                t["torch_ms"].append(window(module, a.iters))
            t["fwd_kernel_ms"].append(window(lambda: run.forward(obs), a.iters))
            t["bwd_kernel_ms"].append(window(lambda: run.bwd_kernel(d), a.iters))
            t["assembly_ms"].append(window(lambda: run.weight_grads(d), a.iters))
            t["assembly_torch_only_ms"].append(window(torch_part, a.iters))
    flop_b = 116.0 * H * H * B * 2
    kb = min(t["bwd_kernel_ms"])
    print(json.dumps(dict(B=B, H=H, nd=a.nd, K=a.K, max_rel_grad_diff_vs_torch_fp32=rel, **t,
                          speedup=min(t["torch_ms"]) / min(t["fused_ms"]), bwd_kernel_tflops=flop_b / (kb * 1e-3) / 1e12,
                          bwd_kernel_x3_ceiling_fraction=flop_b / (kb * 1e-3) / (F16_PEAK / 3))))


if __name__ == "__main__":
    main()
