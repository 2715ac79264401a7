"""fp64 numpy restatement of the reference's QuadsRewardShapingWrapper
(swarm_rl/env_wrappers/reward_shaping.py:19-123) for ONE multi-env of N agents: the expected values of the CPU
fixture test (tests/golden/shaping_*, recorded from the reference's own wrapper) and of the GPU tests.

The wrapper's step() brackets env.step(): begin_step() is what it does before (the scheme reaches rew_coeff on the
first step, :55-61), end_step() what it does with the step's results (:63-121).
"""
import numpy as np

from quadswarm_amd import _native as N
from quadswarm_amd.infos import reward_columns_b

ANNEAL_NAMES = ("quadcol_bin", "quadcol_bin_smooth_max", "quadcol_bin_obst")


def make_scheme(collision_reward, smooth_max, obst_reward, anneal_steps):
    """(reward_shaping_scheme["quad_rewards"], annealing) as make_quadrotor_env_multi builds them
    (swarm_rl/env_wrappers/quad_utils.py:73-91): with annealing the three collision coefficients start at 0.0 and
    each gets a schedule (coeff_name, final_value, anneal_env_steps)."""
    scheme = dict(pos=1.0, effort=0.05, spin=0.1, vel=0.0, crash=1.0, orient=1.0, yaw=0.0,
                  quadcol_bin=collision_reward, quadcol_bin_smooth_max=smooth_max, quadcol_bin_obst=obst_reward)
    annealing = None
    if anneal_steps > 0:
        for k in ANNEAL_NAMES:
            scheme[k] = 0.0
        annealing = [("quadcol_bin", collision_reward, anneal_steps), ("quadcol_bin_smooth_max", smooth_max, anneal_steps),
                     ("quadcol_bin_obst", obst_reward, anneal_steps)]
    return scheme, annealing


class ShapingRestatement:
    def __init__(self, num_agents, rew_coeff, scheme, annealing=None):
        """rew_coeff: the env's (mutable) rew_coeff dict; scheme: reward_shaping_scheme["quad_rewards"];
        annealing: [(coeff_name, final_value, anneal_env_steps)] or None (:20-34)."""
        self.num_agents, self.rew_coeff, self.scheme, self.annealing = num_agents, rew_coeff, scheme, annealing
        self.updated = True
        self.cumulative = None
        self.episode_actions = None

    def reset(self):
        """:46-50"""
        self.cumulative = [dict() for _ in range(self.num_agents)]
        self.episode_actions = []

    def begin_step(self, action):
        """:53-61; returns the rew_coeff the env steps with."""
        self.episode_actions.append(np.asarray(action))
        if self.updated:
            for k, w in self.scheme.items():
                self.rew_coeff[k] = w
            self.updated = False
        return self.rew_coeff

    def end_step(self, rewards, dones, scenario_name, S):
        """:69-121.  rewards: per agent the info["rewards"] dict; dones: per agent; scenario_name: scenario.name()
        AFTER env.step (the in-step reset has run, quadrotor_multi.py:836), or None for an env without scenario;
        S: training_info["approx_total_training_steps"].  Returns per agent None or (true_reward, the dict the
        wrapper merges into episode_extra_stats)."""
        out = [None] * self.num_agents
        for i in range(self.num_agents):
            cum = self.cumulative[i]
            for key, value in rewards[i].items():                                   # :72-76
                if key.startswith("rew"):
                    if key not in cum:
                        cum[key] = 0
                    cum[key] += value
            if dones[i]:
                true_reward = cum["rewraw_main"] + 1000 * cum.get("rewraw_quadcol", 0)   # :79-83
                cum["rewraw_main"] = true_reward                                     # :86
                stats = dict(cum)                                                    # :90
                stats["z_approx_total_training_steps"] = S                           # :92-93
                if scenario_name:                                                    # :95-98
                    for k in ("rew_pos", "rew_crash"):
                        stats[f"{scenario_name}/{k}"] = cum[k]
                ea = np.array(self.episode_actions).transpose()                      # :100-106
                for k in range(ea.shape[0]):
                    stats[f"z_action{k}_mean"] = np.mean(ea[k])
                    stats[f"z_action{k}_std"] = np.std(ea[k])
                self.cumulative[i] = dict()                                          # :108
                if self.annealing:                                                   # :110-118
                    for name, final, steps in self.annealing:
                        self.rew_coeff[name] = min(final * S / steps, final)
                        stats[f"z_anneal_{name}"] = self.rew_coeff[name]
                out[i] = (true_reward, stats)
        if any(dones):                                                               # :120-121
            self.episode_actions = []
        return out


def step_rewards(comp, rew_coeff, final_smooth_max, dt, use_obstacles):
    """The per-agent info["rewards"] dicts of one env's step from its reward components comp [QS_NRI, N] (the step
    kernel's rew_info columns of that env, whose proximity row carries the factor final_smooth_max) under the env's
    own rew_coeff: the proximity term is linear in quadcol_bin_smooth_max (collisions/quadrotors.py:95-103)."""
    c = np.array(comp, dtype=np.float64)
    c[N.RI_PROX] = c[N.RI_PROX] * (rew_coeff["quadcol_bin_smooth_max"] / final_smooth_max) if final_smooth_max else 0.0
    cols = reward_columns_b(c, rew_coeff, dt, use_obstacles)
    return [{k: float(v[i]) for k, v in cols.items()} for i in range(c.shape[1])]


def reward_delta(comp, rew_coeff, final):
    """What an env's own coefficients change in its agents' step reward against the final ones the step kernel ran
    with (fp64, [N]): final = (quadcol_bin, quadcol_bin_smooth_max, quadcol_bin_obst)."""
    c = np.asarray(comp, dtype=np.float64)
    prox = (rew_coeff["quadcol_bin_smooth_max"] / final[1] - 1.0) * c[N.RI_PROX] if final[1] else 0.0
    return ((rew_coeff["quadcol_bin"] - final[0]) * c[N.RI_QUADCOL] + (rew_coeff["quadcol_bin_obst"] - final[2]) * c[N.RI_OBST]
            + prox)
