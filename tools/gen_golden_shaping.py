#!/usr/bin/env python
"""Golden fixtures for the reward shaping wrapper.  TEST INFRASTRUCTURE, dev container only.

    python tools/gen_golden_shaping.py        # writes tests/golden/shaping_*.npz + shaping_*.json

Runs the reference's own QuadsRewardShapingWrapper (swarm_rl/env_wrappers/reward_shaping.py), imported from the
reference tree through tools/refshim.py (stand-ins for sample_factory's TrainingInfoInterface /
RewardShapingInterface), over a scripted stand-in multi-env that carries what the wrapper reads: num_agents,
is_multiagent, unwrapped.rew_coeff, unwrapped.scenario.name(), and a step() that returns scripted
infos[i]["rewards"] dicts and dones.  The stand-in restates:
  * quadrotor_single.py:79-105 / quadrotor_multi.py:642-651: the info["rewards"] keys and how each is formed from
    the raw terms and the env's rew_coeff (quadswarm_amd.infos.reward_columns_b; the key sets are checked against
    the ones recorded from the reference's env, tests/golden/traj_n8info_infokeys.json and
    obst_traj_c4info_infokeys.json), the proximity term being linear in quadcol_bin_smooth_max
    (collisions/quadrotors.py:95-103);
  * quadrotor_multi.py:836: on a done step the env resets itself before step() returns, so scenario.name() is the
    NEXT episode's scenario when the wrapper reads it.
The schedules and the scheme are built as make_quadrotor_env_multi does (quad_utils.py:13-17, 73-91).
Recorded: the scripts (raw terms [T, 8, N] with the proximity row per unit of quadcol_bin_smooth_max, actions
[T, N, 4], dones [T], the scenario name after every step, S before every step), rew_coeff after every step, and for
every done row its true_reward and full episode_extra_stats (key list in the json, values in the npz).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))
import refshim  # noqa: E402

refshim.install()
from swarm_rl.env_wrappers.reward_shaping import DEFAULT_QUAD_REWARD_SHAPING, QuadsRewardShapingWrapper  # noqa: E402

from quadswarm_amd import _native as N  # noqa: E402
from quadswarm_amd.infos import reward_columns_b  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DT = 1.0 / 200.0
COEF3 = ("quadcol_bin", "quadcol_bin_smooth_max", "quadcol_bin_obst")
SCENARIOS = ["Scenario_static_same_goal", "Scenario_dynamic_same_goal", "Scenario_swap_goals", "Scenario_ep_rand_bezier"]
SCENARIOS_OBST = ["Scenario_o_random", "Scenario_o_static_same_goal"]


class AnnealSchedule:   # quad_utils.py:13-17
    def __init__(self, coeff_name, final_value, anneal_env_steps):
        self.coeff_name, self.final_value, self.anneal_env_steps = coeff_name, final_value, anneal_env_steps


class Scenario:
    def __init__(self, names):
        self.names, self.i = names, 0

    def name(self):
        return self.names[self.i % len(self.names)]


class MockMultiEnv:
    """What QuadsRewardShapingWrapper reads of QuadrotorEnvMulti."""
    is_multiagent = True

    def __init__(self, num_agents, comp, dones, scen_names, use_obstacles):
        self.num_agents, self.comp, self.dones, self.use_obstacles = num_agents, comp, dones, use_obstacles
        self.rew_coeff = dict(DEFAULT_QUAD_REWARD_SHAPING["quad_rewards"])   # quad_utils.py:33
        self.scenario = Scenario(scen_names)
        self.t = 0

    @property
    def unwrapped(self):
        return self

    def reset(self):
        return None

    def step(self, action):
        c = np.array(self.comp[self.t], dtype=np.float64)             # [8, N]
        c[N.RI_PROX] = c[N.RI_PROX] * self.rew_coeff["quadcol_bin_smooth_max"]
        cols = reward_columns_b(c, self.rew_coeff, DT, self.use_obstacles)
        infos = [{"rewards": {k: float(v[i]) for k, v in cols.items()}} for i in range(self.num_agents)]
        done = bool(self.dones[self.t])
        self.t += 1
        if done:
            self.scenario.i += 1                                      # quadrotor_multi.py:836 -> :448-459
        return None, [0.0] * self.num_agents, [done] * self.num_agents, infos


def run(name, num_agents, steps, ep_lens, seed, finals=(5.0, 10.0, 5.0), anneal_steps=0.0, s_of_t=None,
        use_obstacles=False):
    rng = np.random.default_rng(seed)
    comp = np.zeros((steps, N.NRI, num_agents))
    comp[:, N.RI_DIST] = rng.uniform(0.0, 4.0, (steps, num_agents))
    comp[:, N.RI_EFFORT] = rng.uniform(0.0, 2.0, (steps, num_agents))
    comp[:, N.RI_CRASH] = rng.uniform(size=(steps, num_agents)) < 0.2
    comp[:, N.RI_ORIENT] = np.where(comp[:, N.RI_CRASH] > 0, 1.0, -rng.uniform(-1.0, 1.0, (steps, num_agents)))
    comp[:, N.RI_SPIN] = rng.uniform(0.0, 10.0, (steps, num_agents))
    comp[:, N.RI_QUADCOL] = -(rng.uniform(size=(steps, num_agents)) < 0.3).astype(np.float64)
    comp[:, N.RI_PROX] = -0.01 * rng.uniform(0.0, 1.0, (steps, num_agents)) * (rng.uniform(size=(steps, num_agents)) < 0.5)
    if use_obstacles:
        comp[:, N.RI_OBST] = -(rng.uniform(size=(steps, num_agents)) < 0.25).astype(np.float64)
    # fp32 values held as fp64: np.mean / np.std (reward_shaping.py:103-104) accumulate in the dtype of the actions
    # they are handed, and the device forms the moments in fp64
    actions = rng.uniform(-1.0, 1.0, (steps, num_agents, 4)).astype(np.float32).astype(np.float64)
    dones = np.zeros(steps, dtype=np.uint8)
    t, k = -1, 0
    while True:
        t += ep_lens[k % len(ep_lens)]
        k += 1
        if t >= steps:
            break
        dones[t] = 1
    S = np.zeros(steps) if s_of_t is None else np.asarray([s_of_t(t) for t in range(steps)], dtype=np.float64)

    env = MockMultiEnv(num_agents, comp, dones, SCENARIOS_OBST if use_obstacles else SCENARIOS, use_obstacles)
    keys_ref = json.load(open(os.path.join(OUT, "obst_traj_c4info_infokeys.json" if use_obstacles
                                           else "traj_n8info_infokeys.json")))["rewards_keys"]
    scheme = {"quad_rewards": dict(DEFAULT_QUAD_REWARD_SHAPING["quad_rewards"])}   # quad_utils.py:73-91
    for c, v in zip(COEF3, finals):
        scheme["quad_rewards"][c] = v
    annealing = None
    if anneal_steps > 0:
        for c in COEF3:
            scheme["quad_rewards"][c] = 0.0
        annealing = [AnnealSchedule(c, v, anneal_steps) for c, v in zip(COEF3, finals)]
    w = QuadsRewardShapingWrapper(env, reward_shaping_scheme=scheme, annealing=annealing, with_pbt=False)
    w.reset()
    coef_after, scen_after, rows = [], [], []
    stat_keys = None
    for t in range(steps):
        w.training_info["approx_total_training_steps"] = float(S[t])
        _, _, d, infos = w.step(actions[t])
        assert sorted(infos[0]["rewards"]) == sorted(keys_ref), "info keys differ from the reference env's"
        coef_after.append([env.rew_coeff[c] for c in COEF3])
        scen_after.append(env.scenario.name())
        for i in range(num_agents):
            if d[i]:
                st = infos[i]["episode_extra_stats"]
                ks = list(st)
                # the scenario-prefixed keys change with the episode: record them per row by position
                if stat_keys is None:
                    stat_keys = [k if not k.startswith("Scenario_") else "<scenario>/" + k.split("/", 1)[1] for k in ks]
                assert [k if not k.startswith("Scenario_") else "<scenario>/" + k.split("/", 1)[1] for k in ks] == stat_keys
                rows.append((t, i, infos[i]["true_reward"], [float(st[k]) for k in ks],
                             [k.split("/", 1)[0] for k in ks if k.startswith("Scenario_")][0]))
    base = os.path.join(OUT, f"shaping_{name}")
    np.savez_compressed(base + ".npz", comp=comp, actions=actions, dones=dones, S=S,
                        coef_after=np.asarray(coef_after, dtype=np.float64),
                        row_t=np.asarray([r[0] for r in rows], dtype=np.int64),
                        row_agent=np.asarray([r[1] for r in rows], dtype=np.int64),
                        row_true_reward=np.asarray([r[2] for r in rows], dtype=np.float64),
                        row_stats=np.asarray([r[3] for r in rows], dtype=np.float64))
    with open(base + ".json", "w") as f:
        json.dump({"name": name, "num_agents": num_agents, "dt": DT, "use_obstacles": use_obstacles,
                   "finals": dict(zip(COEF3, finals)), "anneal_steps": anneal_steps, "coef_names": list(COEF3),
                   "rewards_keys": sorted(keys_ref), "stat_keys": stat_keys, "scenario_after_step": scen_after,
                   "row_scenario": [r[4] for r in rows]}, f, indent=0)
    print(f"{base}: N {num_agents}, {steps} steps, {len(rows)} done rows, {len(stat_keys)} stat keys, "
          f"final coef {coef_after[-1]}")


def main():
    run("n1", 1, 60, [7, 11, 13], seed=1)
    run("n3", 3, 60, [9, 5, 12], seed=2)
    run("n8", 8, 70, [10, 14], seed=3)
    # three schedules, S scripted from 0 past anneal_steps: the clamp at the final value is hit
    run("n2anneal", 2, 90, [6, 9], seed=4, finals=(5.0, 10.0, 4.0), anneal_steps=3000.0, s_of_t=lambda t: 50.0 * t)
    run("obst", 4, 60, [8, 13], seed=5, finals=(5.0, 4.0, 5.0), use_obstacles=True)
    run("obstanneal", 3, 80, [7, 10], seed=6, finals=(5.0, 4.0, 5.0), anneal_steps=2500.0, s_of_t=lambda t: 45.0 * t,
        use_obstacles=True)


if __name__ == "__main__":
    main()
