#!/usr/bin/env python
"""Golden fixtures of flavor B's remaining neighbour observation types (TEST INFRASTRUCTURE, dev container only).

    python tools/gen_golden_nbr.py        # writes tests/golden/neighbors_variants.npz, traj_n4quiet_pos*.npz

From the reference through tools/refshim.py, like tools/gen_golden.py (gen_neighbors_sizes, gen_traj):
  neighbors_variants.npz
      n{n}k{k}_pos / _vel / _rot: random env.pos / .vel / .rot (proper rotations), every fifth case with a
          near-duplicate pair at 1e-3; (8,6), (8,2), (8,7), (32,6), 40 cases each, shared by the types
      {type}_n{n}k{k}_obs: the neighbour block of QuadrotorEnvMulti.add_neighborhood_obs on them for pos and npos;
          pos_Rz, pos_vel_Rz, pos_vel_R in neighbors_variants_{type}[_n8|_n32].npz (file_of: the size limit)
      {type}_low / _high: observation_space.low / .high of one (8,6) env per type, rng3 included
      stale_{type}_{first|after}_pos / _vel / _rot / _obs: what QuadrotorEnvMulti holds after (a) the first reset() of
          a fresh env and (b) reset(), 3 steps, reset(), and the neighbour block that reset returned (n=4, k=2;
          pos_vel_R and pos_Rz)
  traj_n4quiet_pos_vel_R.npz, traj_n4quiet_pos.npz: gen_traj's noise-free hover run (the fields of traj_n8quiet)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (installs the reference shims)

TYPES = ("pos", "npos", "pos_Rz", "pos_vel_Rz", "pos_vel_R")
SIZES = ((8, 6), (8, 2), (8, 7), (32, 6))


def file_of(t, n):
    """The recorded blocks are float64 noise (incompressible), about 3.6 MB in all: the wide types go to files of
    their own so that each stays below the size limit of a committed file.  "" = neighbors_variants.npz."""
    if t in ("pos", "npos"):
        return ""
    return f"_{t}_n{'32' if n > 8 else '8'}" if t == "pos_vel_R" else f"_{t}"


def gen_variants(files, seed=31, count=40):
    """files: file tag -> dict of arrays.  The states of a size are drawn once and shared by the types."""
    rng = np.random.default_rng(seed)
    main = files[""]
    for n, k in SIZES:
        P, V, R = [], [], []
        for c in range(count):
            pos, vel = rng.uniform(-6, 6, (n, 3)), rng.uniform(-4, 4, (n, 3))
            if c % 5 == 0:   # a near-duplicate pair: keys that differ in the low bits
                pos[1] = pos[0] + 1e-3
                vel[1] = vel[0]
            P.append(pos); V.append(vel); R.append(np.stack([G.rand_rot(rng) for _ in range(n)]))
        for name, v in (("pos", P), ("vel", V), ("rot", R)):
            main[f"n{n}k{k}_{name}"] = np.stack(v)
        for t in TYPES:
            env = G.make_env_B(n, k, obs_type=t)
            O = []
            for c in range(count):
                env.pos, env.vel, env.rot = P[c].copy(), V[c].copy(), R[c].copy()
                O.append(np.array(env.add_neighborhood_obs([np.zeros(18) for _ in range(n)]))[:, 18:])
            files[file_of(t, n)][f"{t}_n{n}k{k}_obs"] = np.stack(O)
    for t in TYPES + ("rng3",):
        env = G.make_env_B(8, 6, obs_type=t)
        main[f"{t}_low"] = np.asarray(env.envs[0].observation_space.low)
        main[f"{t}_high"] = np.asarray(env.envs[0].observation_space.high)


def gen_stale(out, seed=32):
    for t in ("pos_vel_R", "pos_Rz"):
        np.random.seed(seed)
        env = G.make_env_B(4, 2, obs_type=t, seed=seed)

        def rec(tag, obs):
            obs = obs[0] if isinstance(obs, tuple) else obs   # (obs, infos)
            out[f"stale_{t}_{tag}_pos"] = np.array(env.pos, dtype=np.float64)
            out[f"stale_{t}_{tag}_vel"] = np.array(env.vel, dtype=np.float64)
            out[f"stale_{t}_{tag}_rot"] = np.array(env.rot, dtype=np.float64)
            out[f"stale_{t}_{tag}_obs"] = np.array(obs, dtype=np.float64)[:, 18:]
        rec("first", env.reset())
        act = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, (3, 4, 4))
        for s in range(3):
            env.step(np.clip(act[s] * 0.6 + 0.3, -1, 1))
        rec("after", env.reset())


def main():
    os.makedirs(G.OUT, exist_ok=True)
    files = {file_of(t, n): {} for t in TYPES for n, _ in SIZES}
    gen_variants(files)
    gen_stale(files[""])
    for tag, out in files.items():
        np.savez_compressed(os.path.join(G.OUT, f"neighbors_variants{tag}.npz"), **out)
    G.gen_traj("n4quiet_pos_vel_R", 4, 2, 100, ep_time=15.0, seed=33, hover=True, sense=None, thrust_noise=0.0,
               obs_type="pos_vel_R")
    G.gen_traj("n4quiet_pos", 4, 2, 100, ep_time=15.0, seed=34, hover=True, sense=None, thrust_noise=0.0,
               obs_type="pos")
    for f in [f"neighbors_variants{tag}.npz" for tag in files] + ["traj_n4quiet_pos_vel_R.npz", "traj_n4quiet_pos.npz"]:
        print(f, os.path.getsize(os.path.join(G.OUT, f)))


if __name__ == "__main__":
    main()
