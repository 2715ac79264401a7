"""Flavor B's neighbour observation types beyond pos_vel (pos, npos, pos_vel_R, pos_Rz, pos_vel_Rz, rng3), the parts
that need no GPU: the numpy restatement (tests/nbr_variants.py) against the reference's recorded blocks, the
observation box, the config / ABI surface, the layouts and the specialised kernels' compilation."""
import ctypes

import numpy as np
import pytest

from nbr_variants import DETERMINISTIC, DIM, golden_file, neighbor_block
from quadswarm_amd import QuadSwarmConfig
from quadswarm_amd import _native as N
from quadswarm_amd.env import observation_bounds

SIX = DETERMINISTIC + ("rng3",)
SIZES = ((8, 6), (8, 2), (8, 7), (32, 6))


@pytest.mark.parametrize("ntype", DETERMINISTIC)
@pytest.mark.parametrize("n,k", SIZES)
def test_restatement_equals_reference(golden, ntype, n, k):
    """QuadrotorEnvMulti.add_neighborhood_obs on 40 random states per size (every fifth with a near-duplicate pair):
    the restatement gives the recorded neighbour block to 1e-12."""
    st, g = golden("neighbors_variants"), golden(golden_file(ntype, n))
    pos, vel, rot = (st[f"n{n}k{k}_{a}"] for a in ("pos", "vel", "rot"))
    want = g[f"{ntype}_n{n}k{k}_obs"]
    assert want.shape == (40, n, k * DIM[ntype])
    for c in range(len(pos)):
        for i in range(n):
            _, rows, order = neighbor_block(ntype, pos[c], vel[c], rot[c], i, k, 10.0)
            np.testing.assert_allclose(rows[order].reshape(-1), want[c, i], rtol=0, atol=1e-12, err_msg=f"case {c} drone {i}")


@pytest.mark.parametrize("ntype", ["pos_vel_R", "pos_Rz"])
@pytest.mark.parametrize("case", ["first", "after"])
def test_restatement_stale_cases(golden, ntype, case):
    """What a reset observes (n=4, k=2): the fresh positions with the velocity and rotation QuadrotorEnvMulti last
    copied at the end of a step -- zero and the identity at the first reset of a fresh env (every R block the
    identity, every Rz block (0, 0, 1)), the previous step's after reset, 3 steps, reset."""
    g = golden("neighbors_variants")
    pos, vel, rot, want = (g[f"stale_{ntype}_{case}_{a}"] for a in ("pos", "vel", "rot", "obs"))
    d = DIM[ntype]
    for i in range(4):
        _, rows, order = neighbor_block(ntype, pos, vel, rot, i, 2, 10.0)
        np.testing.assert_allclose(rows[order].reshape(-1), want[i], rtol=0, atol=1e-12)
    w = want.reshape(4, 2, d)
    if case == "first":
        assert (vel == 0).all() and (rot == np.eye(3)).all()
        tail = np.eye(3).reshape(9) if ntype == "pos_vel_R" else np.array([0.0, 0.0, 1.0])
        assert (w[:, :, d - len(tail):] == tail).all()
        if ntype == "pos_vel_R":
            assert (w[:, :, 3:6] == 0).all()
    else:
        assert np.abs(vel).max() > 1e-3 and np.abs(rot - np.eye(3)).max() > 1e-3


@pytest.mark.parametrize("ntype", SIX)
def test_observation_bounds_equal_reference(golden, ntype):
    g = golden("neighbors_variants")
    cfg = QuadSwarmConfig(num_envs=1, num_agents=8, neighbor_visible_num=6, neighbor_obs_type=ntype)
    lo, hi = observation_bounds(cfg)
    assert lo.dtype == np.float32 and lo.shape == (18 + 6 * DIM[ntype],) == (cfg.obs_dim,)
    np.testing.assert_array_equal(lo, g[f"{ntype}_low"])
    np.testing.assert_array_equal(hi, g[f"{ntype}_high"])


@pytest.mark.parametrize("ntype", SIX)
def test_type_builds_layout_and_specialises(ntype):
    """to_qs_config accepts the type for flavor B; obs_dim = 18 + d k (+ 9 with c4-style obstacles); the hipRTC
    specialisation of its kernels compiles (as test_abi_cpu's obstacle scenarios check theirs)."""
    L = N.lib()
    d = DIM[ntype]
    assert N.NEIGHBOR_DIM[N.NEIGHBOR[ntype]] == d
    for n, k in ((8, 6), (8, 7), (4, 2)):
        cfg = QuadSwarmConfig(num_envs=16, num_agents=n, neighbor_visible_num=k, neighbor_obs_type=ntype)
        qc = cfg.to_qs_config()
        assert qc.neighbor_obs == N.NEIGHBOR[ntype] and qc.abi_version == 16
        lay = N.QsLayout()
        assert L.qs_layout_query(qc, lay) == 0, L.qs_last_error()
        assert lay.obs_dim == 18 + d * k == cfg.obs_dim
    qc = QuadSwarmConfig(num_envs=64, num_agents=8, neighbor_visible_num=6, neighbor_obs_type=ntype).to_qs_config()
    assert L.qs_specialize_compile(qc) > 10000, L.qs_last_error()
    c4 = QuadSwarmConfig.c4(num_envs=64, neighbor_obs_type=ntype)
    lay = N.QsLayout()
    assert L.qs_layout_query(c4.to_qs_config(), lay) == 0, L.qs_last_error()
    assert lay.obs_dim == 19 + d * c4.k_neighbors + 9 == c4.obs_dim


def test_stale_rot_rows_only_where_needed():
    """The stale buffer grows by the 9 rotation rows for the types with an R / Rz part, and for no other."""
    L = N.lib()
    size = {}
    for t in ("pos_vel",) + SIX:
        lay = N.QsLayout()
        qc = QuadSwarmConfig(num_envs=64, num_agents=8, neighbor_visible_num=2, neighbor_obs_type=t).to_qs_config()
        assert L.qs_layout_query(qc, lay) == 0, L.qs_last_error()
        size[t] = lay.obs - lay.stale_vel
    I = 64 * 8
    assert size["pos_vel"] == size["pos"] == size["npos"] == size["rng3"] == 4 * 3 * I
    assert size["pos_vel_R"] == size["pos_Rz"] == size["pos_vel_Rz"] == 4 * 12 * I


def test_lds_budget_counts_the_wider_rows_and_tile():
    """64 drones with all 63 neighbours visible: pos_vel_R stages 64 rows of 963 floats (246 KB, beyond the 160 KB of a
    workgroup) and is refused with the LDS error; pos (207 floats a row) is accepted."""
    L = N.lib()
    lay = N.QsLayout()
    big = QuadSwarmConfig(num_envs=8, num_agents=64, neighbor_visible_num=-1, neighbor_obs_type="pos_vel_R").to_qs_config()
    assert L.qs_layout_query(big, lay) != 0
    assert b"LDS" in L.qs_last_error()
    ok = QuadSwarmConfig(num_envs=8, num_agents=64, neighbor_visible_num=-1, neighbor_obs_type="pos").to_qs_config()
    assert L.qs_layout_query(ok, lay) == 0, L.qs_last_error()
    assert lay.obs_dim == 18 + 3 * 63


@pytest.mark.parametrize("ntype", ["pos_vel_R", "pos_Rz", "pos_vel_Rz", "rng3"])
def test_flavor_a_refuses_the_new_types(ntype):
    with pytest.raises(NotImplementedError):
        QuadSwarmConfig.sb_train(neighbor_obs_type=ntype).to_qs_config()
    qc = QuadSwarmConfig.sb_train(num_envs=4).to_qs_config()
    qc.neighbor_obs = N.NEIGHBOR[ntype]
    assert N.lib().qs_layout_query(qc, N.QsLayout()) != 0


# qs_layout.total_bytes of the pos_vel benchmark configurations before the other types existed
PARENT_TOTAL_BYTES = {"c3": 27793152, "c4": 24516352, "n128": 27082752}


def test_pos_vel_layouts_unchanged():
    cfgs = {"c3": QuadSwarmConfig(num_envs=4096, num_agents=8), "c4": QuadSwarmConfig.c4(),
            "n128": QuadSwarmConfig(num_envs=256, num_agents=128, neighbor_visible_num=6)}
    for name, cfg in cfgs.items():
        lay = N.QsLayout()
        assert N.lib().qs_layout_query(cfg.to_qs_config(), lay) == 0
        assert lay.total_bytes == PARENT_TOTAL_BYTES[name], name
        assert lay.obs - lay.stale_vel == 4 * 3 * cfg.num_envs * cfg.num_agents
