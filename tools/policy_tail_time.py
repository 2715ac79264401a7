#!/usr/bin/env python
"""HIP-event times and launch counts of one rollout policy evaluation with the torch tail against the fused tail
(csrc/qs_policy_tail.h, FusedRolloutPolicy(tail="x3")) on the same inputs in the same process ("the policy
tail").

    python tools/policy_tail_time.py [--B 32768] [--iters 50] [--rounds 3]

Two policies: C3's default (rnn_size 256, identity core, act_dim 4) and sb_train's (rnn_size 128, 6 core layers).  For
each, mha_time.py's method (per round, alternating windows of `iters` back-to-back calls between two events, after
warm-up) on the whole evaluation forward(obs) and on the tail alone (tail() on fixed latents and noise), then, in a
separate pass with the timing done, the device launches of one call of each counted with torch.profiler."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))

import torch  # noqa: E402

from mha_time import window  # noqa: E402
from quadswarm_amd.policy_fused import FusedRolloutPolicy  # noqa: E402
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic  # noqa: E402

POLICIES = {"c3_default": dict(act_dim=4),
            "sb_train": dict(act_dim=4, rnn_size=128, neighbor_hidden_size=128, rnn_type="full", rnn_num_layers=6)}


def launches(fn):
    """Device kernels one call of fn enqueues."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 32768), ("iters", 50), ("rounds", 3)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    for name, kw in POLICIES.items():
        torch.manual_seed(0)
        pc = PolicyConfig(**kw)
        pol = SwarmActorCritic(pc).cuda().eval()
        B, R = a.B, pc.rnn_size
        obs = torch.randn(B, pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs, device="cuda")
        lat = torch.tanh(torch.randn(2, B, 2 * R, device="cuda"))
        noise = torch.randn(B, pc.act_dim, device="cuda")
        fns = {}
        for mode in ("torch", "x3"):
            fp = FusedRolloutPolicy(pol, "x3", tail=mode)
            fp.refresh()
            assert mode == "torch" or fp.packed_tail is not None
            fns["forward_" + mode] = lambda fp=fp: fp(obs)
            fns["tail_" + mode] = lambda fp=fp: fp.tail(lat[0], lat[1], noise)
        diff = max((x - y).abs().max().item() for x, y in zip(fns["tail_x3"](), fns["tail_torch"]()))
        for _ in range(5):
            for f in fns.values():
                f()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                ms[k].append(window(f, a.iters))
        n = {k: launches(f) for k, f in fns.items()}
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps(dict(policy=name, B=B, R=R, n_layers=pc.rnn_num_layers if pc.rnn_type == "full" else 0,
                              ms=ms, launches=n, max_abs_diff_tail_vs_torch_fp32=diff,
                              tail_speedup=best["tail_torch"] / best["tail_x3"],
                              forward_speedup=best["forward_torch"] / best["forward_x3"])))


if __name__ == "__main__":
    main()
