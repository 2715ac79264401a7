#!/usr/bin/env python
"""Time qs_render with HIP events: per-frame time of the two cases DESIGN.md ("Rendering") quotes.

    python tools/render_time.py [--reps 200] [--rounds 7]

Each case: warm-up renders, then `rounds` windows of `reps` back-to-back renders between two events (no host
synchronisation inside a window); the figure is the median window, the spread its min .. max.  One JSON line per case.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import ctypes

    import torch
    from quadswarm_amd import QuadSwarmConfig, _native as N
    from quadswarm_amd.env import QuadSwarmEnv
    from quadswarm_amd.render import RenderConfig

    if not torch.cuda.is_available():
        raise SystemExit("render_time needs the GPU: a time taken elsewhere says nothing")
    L = N.lib()
    cases = [("c3_64envs_256x256", QuadSwarmConfig(num_envs=4096, num_agents=8, specialize=False), 64),
             ("n128_8envs_256x256", QuadSwarmConfig(num_envs=64, num_agents=128, neighbor_visible_num=6, specialize=False), 8)]
    for name, cfg, n in cases:
        env = QuadSwarmEnv(cfg, device=a.device)
        env.reset()
        act = torch.rand(env.I, env.act_dim, device=env.device) * 2 - 1
        env.step_n(act, 20)                                   # a swarm in flight, not the spawn box
        for follow in (False, True):
            rc = RenderConfig(width=256, height=256, view="topdown", follow=follow, drone_scale=4.0)
            ids = list(range(n))
            out = env.render(ids, rc)
            # the timed loop calls the C entry point with prepared arguments: the host must stay ahead of the device
            rcq, idt = rc.to_qs(), torch.tensor(ids, dtype=torch.int32, device=env.device)
            st = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            pi, po = ctypes.c_void_p(idt.data_ptr()), ctypes.c_void_p(out.data_ptr())

            def render():
                N.check(L.qs_render(env._h, ctypes.byref(rcq), pi, n, po, st), "qs_render")
            for _ in range(20):
                render()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    render()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / (a.reps * n))     # us per frame
            times.sort()
            print(json.dumps({"case": name, "follow": follow, "frames_per_call": n, "us_per_frame": round(times[len(times) // 2], 3),
                              "min": round(times[0], 3), "max": round(times[-1], 3),
                              "us_per_call": round(times[len(times) // 2] * n, 2)}), flush=True)
        env.close()


if __name__ == "__main__":
    main()
