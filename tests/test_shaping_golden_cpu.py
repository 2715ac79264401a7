"""The reward shaping wrapper on the CPU: tests/shaping_restatement.py and quadswarm_amd.stats.shaping_infos against
fixtures recorded from the reference's own QuadsRewardShapingWrapper (tools/gen_golden_shaping.py), and the config
surface.  No GPU."""
import glob
import json
import os
import types

import numpy as np
import pytest

from quadswarm_amd import QuadSwarmConfig, _native as N
from quadswarm_amd.stats import shaping_infos
from shaping_restatement import ShapingRestatement, make_scheme

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[len("shaping_"):-len(".json")] for p in glob.glob(os.path.join(GOLD, "shaping_*.json")))


def load(name):
    meta = json.load(open(os.path.join(GOLD, f"shaping_{name}.json")))
    return meta, np.load(os.path.join(GOLD, f"shaping_{name}.npz"))


def row_keys(meta, k):
    return [s.replace("<scenario>", meta["row_scenario"][k]) for s in meta["stat_keys"]]


def test_fixture_set():
    # N = 1, 3, 8 without annealing, N = 2 with the three schedules, the obstacle key set
    assert {"n1", "n3", "n8", "n2anneal", "obst"} <= set(NAMES)
    meta, z = load("n2anneal")
    f = meta["finals"]
    ca = z["coef_after"]
    assert (ca[0] == 0).all(), "with annealing every env starts its first episode at 0 (quad_utils.py:80-83)"
    assert (ca[-1] == [f[c] for c in meta["coef_names"]]).all(), "S passes anneal_steps: the clamp at final is hit"
    assert ((ca > 0) & (ca < ca[-1])).any(), "and values strictly inside (0, final) occur"
    assert len(load("obst")[0]["rewards_keys"]) == 17 and len(load("n8")[0]["rewards_keys"]) == 15


def replay(meta, z):
    """The restatement over a fixture's scripts, the stand-in env's reward dicts restated as the generator forms them."""
    from quadswarm_amd.infos import reward_columns_b
    n, f = meta["num_agents"], meta["finals"]
    scheme, annealing = make_scheme(f["quadcol_bin"], f["quadcol_bin_smooth_max"], f["quadcol_bin_obst"], meta["anneal_steps"])
    rew_coeff = dict(pos=1.0, effort=0.05, spin=0.1, vel=0.0, crash=1.0, orient=1.0, yaw=0.0,
                     quadcol_bin=0.0, quadcol_bin_smooth_max=0.0, quadcol_bin_obst=0.0)   # reward_shaping.py:7-16
    r = ShapingRestatement(n, rew_coeff, scheme, annealing)
    r.reset()
    rows, coef_after = [], []
    for t in range(len(z["dones"])):
        c = r.begin_step(z["actions"][t])
        comp = np.array(z["comp"][t])
        comp[N.RI_PROX] = comp[N.RI_PROX] * c["quadcol_bin_smooth_max"]
        cols = reward_columns_b(comp, c, meta["dt"], meta["use_obstacles"])
        rewards = [{k: float(v[i]) for k, v in cols.items()} for i in range(n)]
        out = r.end_step(rewards, [bool(z["dones"][t])] * n, meta["scenario_after_step"][t], float(z["S"][t]))
        rows += [(t, i) + out[i] for i in range(n) if out[i] is not None]
        coef_after.append([rew_coeff[k] for k in meta["coef_names"]])
    return rows, np.asarray(coef_after)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_replays_fixture(name):
    meta, z = load(name)
    rows, coef_after = replay(meta, z)
    assert (coef_after == z["coef_after"]).all(), "rew_coeff after every step is exactly the reference's"
    assert [(t, i) for t, i, _, _ in rows] == list(zip(z["row_t"].tolist(), z["row_agent"].tolist()))
    for k, (t, i, tr, st) in enumerate(rows):
        keys = row_keys(meta, k)
        assert sorted(st) == sorted(keys), f"row {k}"
        np.testing.assert_allclose(tr, z["row_true_reward"][k], rtol=1e-12, atol=0)
        np.testing.assert_allclose([st[q] for q in keys], z["row_stats"][k], rtol=1e-12, atol=0, err_msg=f"row {k}")
        assert st["rewraw_main"] == tr


@pytest.mark.parametrize("name", NAMES)
def test_stats_row_to_dict(name):
    """shaping_infos on rows built from the fixture's own per-step scripts, the way the kernel builds them: raw sums
    (proximity at the final coefficient's scale), the coefficients in force, the next ones, S, the action moments,
    the scenario AFTER the step.  It forms coefficient x (sum of raw terms) where the reference sums coefficient x
    raw term, so the two differ by fp64 rounding only: up to n + 1 roundings of relative size 2^-53 on a sum of n
    <= 14 same-sign terms, far inside rtol 1e-12; rew_orient mixes signs, so its bound is taken on the sum of the
    magnitudes (atol 1e-12 x 14 steps x dt x 1 = 7e-14 at most, 1e-13 used)."""
    from quadswarm_amd.stats import SCENARIO_NAMES
    meta, z = load(name)
    n, f, dt = meta["num_agents"], meta["finals"], meta["dt"]
    fin = [f[c] for c in meta["coef_names"]]
    ann = meta["anneal_steps"] > 0
    coeff = dict(pos=1.0, effort=0.05, crash=1.0, orient=1.0, spin=0.1, quadcol_bin=fin[0], quadcol_bin_obst=fin[2],
                 quadcol_bin_smooth_max=fin[1])
    ids = {"Scenario_" + v: k for k, v in SCENARIO_NAMES.items()}
    start, k = 0, 0
    for t in np.nonzero(z["dones"])[0]:
        assert t > start
        used = z["coef_after"][start]                             # constant within an episode (:110-118)
        a = z["actions"][start:t + 1].astype(np.float64)          # [T, N, 4]
        for i in range(n):
            row = np.zeros(N.NSH)
            comp = z["comp"][start:t + 1, :, i].sum(0)
            comp[N.RI_PROX] *= fin[1]
            row[N.SH_SUM:N.SH_SUM + 8] = comp
            row[N.SH_COEF:N.SH_COEF + 3] = used
            row[N.SH_ANNEAL:N.SH_ANNEAL + 3] = z["coef_after"][t]
            row[N.SH_S] = z["S"][t]
            for q in range(4):
                row[N.SH_ACT_MEAN + q], row[N.SH_ACT_STD + q] = a[:, :, q].mean(), a[:, :, q].std()
            row[N.SH_LEN] = t + 1 - start
            row[N.SH_SCEN] = ids[meta["scenario_after_step"][t]]
            tr, st = shaping_infos(row, coeff, dt, meta["use_obstacles"], annealing=ann)
            assert (int(z["row_t"][k]), int(z["row_agent"][k])) == (int(t), i)
            keys = row_keys(meta, k)
            assert sorted(st) == sorted(keys)
            assert meta["scenario_after_step"][t] + "/rew_pos" in st      # the NEXT episode's scenario
            assert st["rewraw_main"] == tr
            np.testing.assert_allclose(tr, z["row_true_reward"][k], rtol=1e-12, atol=0)
            np.testing.assert_allclose([st[q] for q in keys], z["row_stats"][k], rtol=1e-12, atol=1e-13, err_msg=f"row {k}")
            k += 1
        start = t + 1
    assert k == len(z["row_t"])


def test_scenario_key_is_the_next_episodes():
    meta, z = load("n8")
    t = int(np.nonzero(z["dones"])[0][0])
    assert meta["scenario_after_step"][t] != meta["scenario_after_step"][t - 1]
    assert meta["row_scenario"][0] == meta["scenario_after_step"][t]


def test_config_surface():
    with pytest.raises(KeyError, match="rewraw_main"):
        QuadSwarmConfig.sb_train(num_envs=2, reward_shaping=True).validate()
    with pytest.raises(ValueError):
        QuadSwarmConfig(num_envs=2, reward_shaping=True, anneal_collision_steps=-1.0).validate()
    c = QuadSwarmConfig(num_envs=2, reward_shaping=True, anneal_collision_steps=3e8)
    q = c.to_qs_config()
    assert q.step_infos == 1, "the wrapper reads rew_info: reward_shaping turns step_infos on"
    assert QuadSwarmConfig(num_envs=2).to_qs_config().step_infos == 0
    # with obstacles the row's scenario id is an env word the kernels keep with the episode stats
    assert QuadSwarmConfig.c4(num_envs=2, reward_shaping=True, episode_stats=False).to_qs_config().episode_stats == 1
    assert QuadSwarmConfig.c4(num_envs=2, episode_stats=False).to_qs_config().episode_stats == 0
    assert QuadSwarmConfig(num_envs=2, reward_shaping=True, episode_stats=False).to_qs_config().episode_stats == 0
    ref = types.SimpleNamespace(quads_num_agents=8, anneal_collision_steps=300000000.0)
    assert QuadSwarmConfig.from_reference_cfg(ref).anneal_collision_steps == 3e8
    assert QuadSwarmConfig.from_reference_cfg(types.SimpleNamespace()).anneal_collision_steps == 0.0


def test_abi_additions():
    L = N.lib()
    assert L.qs_abi_version() == 16
    sc = N.QsShapingConfig(anneal_steps=5.0)
    assert L.qs_shaping_config_default(sc) == 0 and sc.anneal_steps == 0.0
    assert L.qs_shaping_config_default(None) == -1
    assert L.qs_shaping_enable(None, sc, None) == -1
    assert N.NSH % 4 == 0 and N.SH_REW < N.NSH
