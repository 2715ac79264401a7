#!/usr/bin/env python
"""Time the reward shaping kernel with HIP events: what a step costs with the wrapper on, next to the same step without.

    python tools/shaping_time.py [--reps 10000] [--rounds 7]

Each case runs one handle with shaping and one without, same config and actions: warm-up steps, then `rounds`
windows of `reps` back-to-back qs_step_n steps between two events (no host synchronisation inside a window),
alternating the two handles window by window so both see the same clocks.  The figure is the median window, the
spread its min .. max.  One JSON line per case; DESIGN.md ("Reward shaping") quotes them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import torch
    from quadswarm_amd import QuadSwarmConfig
    from quadswarm_amd.env import QuadSwarmEnv

    if not torch.cuda.is_available():
        raise SystemExit("shaping_time needs the GPU: a time taken elsewhere says nothing")
    cases = [("c3_4096x8", lambda: QuadSwarmConfig(num_envs=4096, num_agents=8, step_infos=True), 0.0),
             ("c3_4096x8_anneal", lambda: QuadSwarmConfig(num_envs=4096, num_agents=8, step_infos=True), 3e8),
             ("c4_4096x8_anneal", lambda: QuadSwarmConfig.c4(num_envs=4096, step_infos=True), 3e8),
             ("n128_256x128", lambda: QuadSwarmConfig(num_envs=256, num_agents=128, neighbor_visible_num=6,
                                                      step_infos=True), 0.0)]
    for name, mk, anneal in cases:
        envs = {"off": QuadSwarmEnv(mk(), device=a.device), "on": QuadSwarmEnv(mk(), device=a.device)}
        envs["on"].enable_reward_shaping(anneal)
        act = torch.rand(envs["on"].I, 4, device=envs["on"].device) * 2 - 1
        for e in envs.values():
            e.reset()
            e.step_n(act, 50)
        torch.cuda.synchronize()
        times = {"off": [], "on": []}
        for _ in range(a.rounds):
            for k, e in envs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                e.step_n(act, a.reps)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)     # us per step
        out = {"case": name, "anneal_steps": anneal, "reps": a.reps, "rounds": a.rounds}
        for k, v in times.items():
            v.sort()
            out[f"us_per_step_{k}"] = round(v[len(v) // 2], 3)
            out[f"min_{k}"], out[f"max_{k}"] = round(v[0], 3), round(v[-1], 3)
        out["shaping_us"] = round(out["us_per_step_on"] - out["us_per_step_off"], 3)
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
