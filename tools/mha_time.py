#!/usr/bin/env python
"""HIP-event time of the fused multi-head attention encoder (csrc/qs_policy_mha.h) next to the torch module's encoder
tokens on the same inputs in the same process ("multi-head attention encoder").

    python tools/mha_time.py [--B 32768] [--H 256] [--nd 6] [--K 6] [--iters 50] [--rounds 3]

Per round, alternating: `iters` two-tower kernel launches, then `iters` torch evaluations of both towers' tokens, each
window between two events.  FLOP from the shapes: per agent and tower 2 (34 H^2 + 160 H) (layer 0 on 80 columns, layer
1, 4 heads x (q, k, v, fc), two token rows); the x3 ceiling is the f16 matrix peak / 3 (three MFMAs per product)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))

import torch  # noqa: E402

from quadswarm_amd.policy_fused import FusedRolloutPolicy  # noqa: E402
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic  # noqa: E402

F16_PEAK = 2.5e15   # MI355X dense f16 matrix rate, FLOP/s


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 32768), ("H", 256), ("nd", 6), ("K", 6), ("iters", 50), ("rounds", 3)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    torch.manual_seed(0)
    pc = PolicyConfig(self_obs_dim=19, neighbor_obs_dim=a.nd, num_use_neighbor_obs=a.K, obstacle_obs_dim=9, rnn_size=a.H,
                      neighbor_hidden_size=a.H, act_dim=4, encoder_type="attention")
    pol = SwarmActorCritic(pc).cuda().eval()
    obs = torch.randn(a.B, 19 + a.nd * a.K + 9, device="cuda")
    fp = FusedRolloutPolicy(pol, "x3")
    encs = (pol.actor_encoder, pol.critic_encoder)
    with torch.no_grad():
        kernel = lambda: fp.neighbor_encodings(obs)  # noqa: E731
        module = lambda: [e.tokens(obs) for e in encs]  # noqa: E731
        diff = max((k - m).abs().max().item() for k, m in zip(kernel(), module()))
        for _ in range(5):
            kernel()
            module()
        tk, tm = [], []
        for _ in range(a.rounds):
            tk.append(window(kernel, a.iters))
            tm.append(window(module, a.iters))
    flop = 2.0 * (34 * a.H * a.H + 160 * a.H) * a.B * 2
    best = min(tk)
    print(json.dumps(dict(B=a.B, H=a.H, nd=a.nd, K=a.K, kernel_ms=tk, torch_ms=tm, max_abs_diff_vs_torch_fp32=diff,
                          flop=flop, kernel_tflops=flop / (best * 1e-3) / 1e12,
                          x3_ceiling_fraction=flop / (best * 1e-3) / (F16_PEAK / 3))))


if __name__ == "__main__":
    main()
