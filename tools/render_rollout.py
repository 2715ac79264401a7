#!/usr/bin/env python
"""Roll a policy (a PPOTrainer checkpoint, or random actions) and write what the swarm does as pictures: the
counterpart of the reference's swarm_rl/sb_render.py without a display.  Every step the chosen envs are drawn on the
device (QuadSwarmEnv.render -> qs_render); the frames reach the host once, at the end.

    python tools/render_rollout.py --config c3 --frames 200 --out out/c3 [--checkpoint run/ckpt.pt]
        [--envs 0,1,2,3] [--view topdown|side|front] [--follow] [--size 256x256] [--drone-scale 4] [--every 1]

Writes <out>/frames.npy [T, H, W, 3] uint8 (the chosen envs tiled like SB3's tile_images) and <out>/frame_00000.png ...
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))


def make_config(name, num_envs, seed):
    from quadswarm_amd import QuadSwarmConfig
    if name == "c3":
        return QuadSwarmConfig(num_envs=num_envs, num_agents=8, seed=seed)
    if name == "c4":
        return QuadSwarmConfig.c4(num_envs=num_envs, seed=seed)
    if name == "sb_train":
        return QuadSwarmConfig.sb_train(num_envs=num_envs, num_agents=8, seed=seed)
    if name == "n128":
        return QuadSwarmConfig(num_envs=num_envs, num_agents=128, neighbor_visible_num=6, seed=seed)
    raise SystemExit(f"unknown config {name!r}: c3, c4, sb_train or n128")


def load_policy(path, env_cfg, device):
    import torch
    from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic
    ck = torch.load(path, map_location="cpu", weights_only=True)
    pc = PolicyConfig(**ck["policy_cfg"])
    want = PolicyConfig.for_env(env_cfg)
    if (pc.self_obs_dim, pc.neighbor_obs_dim, pc.num_use_neighbor_obs, pc.obstacle_obs_dim, pc.act_dim) != \
            (want.self_obs_dim, want.neighbor_obs_dim, want.num_use_neighbor_obs, want.obstacle_obs_dim, want.act_dim):
        raise SystemExit("the checkpoint's policy was trained on another observation / action layout than --config")
    policy = SwarmActorCritic(pc).to(device)
    policy.load_state_dict(ck["policy"])
    return policy.eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--checkpoint", default=None, help="PPOTrainer.save file; without it the actions are uniform noise")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--every", type=int, default=1, help="env steps per frame")
    ap.add_argument("--num-envs", type=int, default=16)
    ap.add_argument("--envs", default="0", help="comma-separated env indices to draw")
    ap.add_argument("--view", default="topdown")
    ap.add_argument("--follow", action="store_true")
    ap.add_argument("--size", default="256x256", help="WIDTHxHEIGHT of one env's frame")
    ap.add_argument("--drone-scale", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True)
    ap.add_argument("--no-png", action="store_true")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    from quadswarm_amd.env import QuadSwarmEnv
    from quadswarm_amd.render import RenderConfig, tile_images, write_png

    w, h = (int(v) for v in a.size.lower().split("x"))
    ids = [int(v) for v in a.envs.split(",")]
    rc = RenderConfig(width=w, height=h, view=a.view, follow=a.follow, drone_scale=a.drone_scale)
    cfg = make_config(a.config, max(a.num_envs, max(ids) + 1), a.seed)
    env = QuadSwarmEnv(cfg, device=a.device)
    policy = load_policy(a.checkpoint, cfg, env.device) if a.checkpoint else None
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    frames = torch.empty(a.frames, len(ids), h, w, 3, dtype=torch.uint8, device=env.device)
    obs = env.reset()
    with torch.no_grad():
        for t in range(a.frames):
            env.render(ids, rc, out=frames[t])
            for _ in range(a.every):
                if policy is not None:
                    act = policy.predict(obs, deterministic=True)
                else:
                    act = torch.rand(env.I, env.act_dim, generator=gen, device=env.device) * 2 - 1
                obs = env.step(act.contiguous())[0]
    host = frames.cpu().numpy()                       # the one copy to the host
    env.close()
    tiled = np.stack([tile_images(f) for f in host])
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "frames.npy"), tiled)
    if not a.no_png:
        for t, f in enumerate(tiled):
            write_png(os.path.join(a.out, f"frame_{t:05d}.png"), f)
    print(f"{a.frames} frames {tiled.shape[2]} x {tiled.shape[1]} of envs {ids} -> {a.out}")


if __name__ == "__main__":
    main()
