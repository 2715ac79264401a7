"""Flavor B's neighbour observation types beyond pos_vel on the GPU: pos, npos, pos_vel_R, pos_Rz, pos_vel_Rz against
the numpy restatement (tests/nbr_variants.py, pinned to the reference by test_neighbor_variants_cpu.py) on the
oracle's states, rng3 as noise, every type against its pos_vel twin (no draw moved), the specialised kernels against
the generic ones, the reference's own trajectories, and the replay snapshot.  Needs an MI355X.

The oracle (oracle_params reads only k_neighbors) runs unchanged: its own pos_vel block is ignored, its state,
rewards, done flags and self obs are the reference of everything but the neighbour block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import oracle as O  # noqa: E402
from nbr_variants import DETERMINISTIC, DIM, assert_nbr_match  # noqa: E402
from parity_utils import crowd, oracle_params, oracle_state_arrays, oracle_to_gpu  # noqa: E402
from quadswarm_amd import QuadSwarmConfig  # noqa: E402
from quadswarm_amd import _native as N_  # noqa: E402
from quadswarm_amd.env import QuadSwarmEnv  # noqa: E402
from test_gpu_parity import (QUIET_OBS, QUIET_OMEGA, QUIET_STATE, _close_rows, _load_initial_state,  # noqa: E402
                             eventful_rows)
from test_gpu_specialize import assert_same  # noqa: E402

ROOM = 10.0
ROT_TYPES = ("pos_vel_R", "pos_Rz", "pos_vel_Rz")
SIX = DETERMINISTIC + ("rng3",)


def np_(t):
    return t.double().cpu().numpy()


def make_pair(ntype, E, N, K, seed=7, **kw):
    cfg = QuadSwarmConfig(num_envs=E, num_agents=N, neighbor_visible_num=K, neighbor_obs_type=ntype, seed=seed, **kw)
    env = QuadSwarmEnv(cfg)
    oenv = O.OracleEnv(oracle_params(cfg), seed=seed)
    return cfg, env, oenv


RESET_CASES = [(t, n, k) for t in DETERMINISTIC for n, k in ((8, 6), (8, 7), (4, 2))] + \
              [("pos_vel_R", n, 6) for n in (32, 64, 128)]


@pytest.mark.parametrize("ntype,N,K", RESET_CASES)
def test_reset_matches_restatement(ntype, N, K):
    """The first reset of a fresh env: self obs as test_reset_matches_oracle, the neighbour block = the restatement
    of the fresh positions with velocity zero and rotation the identity (QuadrotorEnvMulti.vel / .rot before any
    step, quadrotor_multi.py:92-95), not the freshly drawn yaw."""
    cfg, env, oenv = make_pair(ntype, 512 // N, N, K)
    obs = np_(env.reset())
    want = oenv.reset()
    assert obs.shape == (env.I, 18 + DIM[ntype] * K)
    np.testing.assert_allclose(obs[:, :18], want[:, :18], atol=2e-5, rtol=1e-5)
    pos = np.array([oenv.drones[g].pos[:] for g in range(env.I)])
    rot = np.broadcast_to(np.eye(3), (env.I, 3, 3))
    assert_nbr_match(obs[:, 18:], ntype, pos, np.zeros((env.I, 3)), rot, N, K, ROOM)
    if ntype in ROT_TYPES:
        np.testing.assert_array_equal(np_(env.stale_rot).T.reshape(env.I, 3, 3), rot)
        assert np.abs(np_(env.drone_fields()["rot"]) - rot).max() > 0.1    # the drones themselves are yawed
    else:
        assert env.stale_rot is None


@pytest.mark.parametrize("ntype", ["pos_vel_R", "pos_Rz"])
@pytest.mark.parametrize("N,K", [(8, 6), (64, 6)])
def test_reset_after_steps_sees_stale_vel_and_rot(ntype, N, K):
    """reset, 3 random steps, reset: the block is the restatement of the fresh positions with the velocity and the
    rotation the last step left (the same fp32 inputs on both sides: 2e-5)."""
    cfg, env, _ = make_pair(ntype, 512 // N, N, K)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(3):
        _, _, done, _ = env.step((torch.rand(env.I, 4, device="cuda", generator=g) * 2 - 1).contiguous())
        assert not done.any()
    f = env.drone_fields()
    vel, rot = np_(f["vel"]), np_(f["rot"])
    obs = np_(env.reset())
    pos = np_(env.drone_fields()["pos"])
    assert np.abs(vel).max() > 1e-2 and np.abs(rot - np.eye(3)).max() > 1e-2
    assert_nbr_match(obs[:, 18:], ntype, pos, vel, rot, N, K, ROOM, atol=2e-5, rtol=1e-5)
    np.testing.assert_array_equal(np_(env.stale_rot).T.reshape(env.I, 3, 3), rot)
    # a second reset in a row still sees them (reset refreshes only the positions)
    obs = np_(env.reset())
    assert_nbr_match(obs[:, 18:], ntype, np_(env.drone_fields()["pos"]), vel, rot, N, K, ROOM, atol=2e-5, rtol=1e-5)


STEP_CASES = [(t, 8, k, False) for t in DETERMINISTIC for k in (6, 7)] + \
             [("pos_vel_R", 32, 6, False), ("pos_vel_R", 64, 6, False), ("pos_vel_R", 128, 6, False),
              ("pos_vel_R", 8, 2, True)]


@pytest.mark.parametrize("ntype,N,K,dw", STEP_CASES)
def test_one_step_from_identical_state(ntype, N, K, dw):
    """The loop of test_gpu_parity.py::test_one_step_from_identical_state (crowded envs, 12 steps, auto-resets),
    the neighbour block against the restatement of the oracle's post-step QuadrotorEnvMulti.pos / .vel / .rot: for
    an env that finished, the fresh positions with the finished step's velocity (the oracle's obs_vel) and rotation
    (columns 6:15 of its terminal self obs: sense_noise=None for the types that read the rotation).

    Rows whose fp32 selection differs from the fp64 one on these states (nbr_variants.selection_diffs on the
    oracle's states of the same runs, CPU): 0 of 6144 for every case below (cap: 61)."""
    E = 512 // N
    kw = dict(sense_noise=None) if ntype in ROT_TYPES else {}
    cfg, env, oenv = make_pair(ntype, E, N, K, use_downwash=dw, episode_duration=0.5, **kw)
    d = DIM[ntype]
    env.reset()
    oenv.reset()
    rng = np.random.default_rng(3)
    crowd(oenv, rng)
    obs_rot = np.broadcast_to(np.eye(3).reshape(9), (env.I, 9)).copy()   # QuadrotorEnvMulti.rot after the first reset
    stats = dict(done=0, quiet=0, eventful=0)
    for t in range(12):
        oracle_to_gpu(oenv, env)
        if env.stale_rot is not None:
            env.stale_rot.copy_(torch.from_numpy(obs_rot.T.astype(np.float32).copy()))
        floor_before = np.array([oenv.drones[g].on_floor != 0 for g in range(env.I)])
        a = rng.uniform(-1, 1, (env.I, 4)).astype(np.float32)
        obs, rew, done, term = env.step(torch.from_numpy(a).cuda())
        w_obs, w_rew, w_done, w_term = oenv.step(a.astype(np.float64))
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), w_done)
        loud = eventful_rows(oenv, floor_before, w_done)
        quiet = ~loud
        stats["quiet"] += int(quiet.sum())
        stats["eventful"] += int(loud.sum())
        g_rew, g_obs = np_(rew), np_(obs)
        assert g_obs.shape[1] == 18 + d * K
        np.testing.assert_allclose(g_rew, w_rew, atol=2e-4, rtol=1e-4)
        _close_rows(g_rew, w_rew, quiet, f"step {t} quiet rew", **QUIET_STATE)
        np.testing.assert_allclose(g_obs[:, :18], w_obs[:, :18], atol=2e-4, rtol=1e-4)
        _close_rows(g_obs[:, :15], w_obs[:, :15], quiet, f"step {t} quiet self obs", **QUIET_OBS)
        _close_rows(g_obs[:, 15:18], w_obs[:, 15:18], quiet, f"step {t} quiet obs omega", **QUIET_OMEGA)
        pos, vel, rot, _ = oracle_state_arrays(oenv)
        obs_rot = np.where(w_done[:, None], w_term[:, 6:15], rot)
        P = np.array([oenv.envs[g // N].obs_pos[g % N][:] for g in range(env.I)])
        V = np.array([oenv.envs[g // N].obs_vel[g % N][:] for g in range(env.I)])
        assert_nbr_match(g_obs[:, 18:], ntype, P, V, obs_rot.reshape(-1, 3, 3), N, K, ROOM)
        if w_done.any():
            np.testing.assert_allclose(np_(term)[w_done, :18], w_term[w_done, :18], atol=2e-4, rtol=1e-4)
        stats["done"] += int(w_done.sum())
        f = env.drone_fields()
        np.testing.assert_allclose(np_(f["pos"]), pos, atol=2e-5)
        np.testing.assert_allclose(np_(f["vel"]), vel, atol=5e-4, rtol=1e-4)
        for k, want in (("pos", pos), ("vel", vel), ("rot", rot)):
            _close_rows(np_(f[k]).reshape(env.I, -1), want, quiet, f"step {t} quiet {k}", **QUIET_STATE)
    assert stats["done"] > 0
    assert stats["quiet"] > stats["eventful"] > 0, stats


def _run(env, steps, seed=11, reset_at=None):
    """reset + `steps` random steps (an explicit reset before step reset_at); the outputs of every call."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = [dict(obs=env.reset().clone())]
    for t in range(steps):
        if t == reset_at:
            out.append(dict(obs=env.reset().clone()))
        a = (torch.rand(env.I, 4, device="cuda", generator=g) * 2 - 1).contiguous()
        obs, rew, done, term = env.step(a)
        out.append(dict(obs=obs.clone(), rew=rew.clone(), done=done.clone(), term=term.clone()))
    return out


@pytest.mark.parametrize("ntype", SIX)
def test_twin_of_pos_vel_is_bitwise_equal(ntype):
    """The same seed and actions with pos_vel and with the type, 40 steps with auto-resets and an explicit reset:
    state, istate, env_state, rewards, done flags and the self obs are bitwise equal -- the neighbour type changes
    the neighbour block alone and moves no draw (rng3's own stream included)."""
    envs = [QuadSwarmEnv(QuadSwarmConfig(num_envs=64, num_agents=8, neighbor_visible_num=6, neighbor_obs_type=t,
                                         episode_duration=0.3, seed=4)) for t in ("pos_vel", ntype)]
    a, b = (_run(e, 40, reset_at=35) for e in envs)
    dones = 0
    for t, (x, y) in enumerate(zip(a, b)):
        assert_same(y["obs"][:, :18], x["obs"][:, :18], f"self obs call {t}")
        if "rew" in x:
            assert_same(y["rew"], x["rew"], f"rew call {t}")
            assert_same(y["done"], x["done"], f"done call {t}")
            assert_same(y["term"][:, :18], x["term"][:, :18], f"terminal self obs call {t}")
            dones += int(x["done"].sum())
    assert dones > 0
    assert_same(envs[1].state, envs[0].state, "state")
    assert torch.equal(envs[1].istate, envs[0].istate) and torch.equal(envs[1].env_state, envs[0].env_state)
    assert_same(envs[1].stale_vel, envs[0].stale_vel, "stale_vel")


def test_rng3_is_noise():
    """rng3 (np.random.rand(3) per slot): every value in [0, 1), no block repeated across drones or steps, a function
    of the seed, and uniform: the mean of n values has standard deviation 1 / sqrt(12 n), the bound is 5 of them."""
    def blocks(seed):
        env = QuadSwarmEnv(QuadSwarmConfig(num_envs=64, num_agents=8, neighbor_visible_num=6, neighbor_obs_type="rng3",
                                           seed=seed))
        return torch.stack([o["obs"][:, 18:] for o in _run(env, 20)]).cpu()
    a, b, c = blocks(3), blocks(3), blocks(4)
    assert a.shape == (21, 512, 18)
    assert (a >= 0).all() and (a < 1).all()
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and (a != c).float().mean() > 0.99
    rows = a.reshape(-1, 18).numpy()
    assert len(np.unique(rows, axis=0)) == len(rows)
    assert len(np.unique(rows.reshape(-1, 3), axis=0)) == rows.size // 3     # no slot repeated either
    n = rows.size
    assert abs(rows.astype(np.float64).mean() - 0.5) <= 5.0 / np.sqrt(12.0 * n)


SPEC = {
    "pos_mix": lambda: QuadSwarmConfig(num_envs=512, num_agents=4, neighbor_visible_num=3, neighbor_obs_type="pos",
                                       quads_mode="mix", episode_duration=0.3, seed=4),
    "pos_vel_R": lambda: QuadSwarmConfig(num_envs=512, num_agents=8, neighbor_visible_num=6, neighbor_obs_type="pos_vel_R",
                                         episode_duration=0.3, seed=4),
    "pos_Rz_n32": lambda: QuadSwarmConfig(num_envs=64, num_agents=32, neighbor_visible_num=6, neighbor_obs_type="pos_Rz",
                                          episode_duration=0.3, seed=4),
}


@pytest.mark.parametrize("name", sorted(SPEC))
def test_specialised_matches_generic(name):
    """The loop of test_gpu_specialize.py::test_specialised_matches_generic: bitwise."""
    cfg = SPEC[name]()
    cfg.specialize = False
    gen = QuadSwarmEnv(cfg)
    spc = QuadSwarmEnv(SPEC[name]())
    spc.specialize(True)
    assert spc.specialized and not gen.specialized
    assert_same(spc.reset(), gen.reset(), "reset obs")
    g = torch.Generator(device="cuda").manual_seed(11)
    dones = 0
    for t in range(40):
        a = (torch.rand(gen.I, 4, device="cuda", generator=g) * 2 - 1).contiguous()
        if t == 20:
            for e in (gen, spc):
                e.set_param("rew_pos", 2.0)
        r1, r2 = gen.step(a), spc.step(a)
        for x, y, w in zip(r2, r1, ("obs", "rew", "done", "term")):
            assert_same(x, y, f"{w} step {t}")
        dones += int(r1[2].sum())
    assert_same(spc.state, gen.state, "state")
    assert torch.equal(spc.istate, gen.istate) and torch.equal(spc.env_state, gen.env_state)
    assert_same(spc.stale_vel, gen.stale_vel, "stale_vel")
    if gen.stale_rot is not None:
        assert_same(spc.stale_rot, gen.stale_rot, "stale_rot")
    assert dones > 0


def _neighbors_close(got, want, d, atol):
    """test_gpu_parity.assert_neighbors_close for slots of d floats: compared up to a permutation."""
    got, want = got.reshape(len(got), -1, d), want.reshape(len(want), -1, d)
    for i in range(len(got)):
        dist = np.abs(got[i][:, None, :] - want[i][None, :, :]).max(-1)
        match = dist.argmin(1)
        assert len(set(match.tolist())) == len(match), f"drone {i}: neighbour sets differ"
        assert dist[np.arange(len(match)), match].max() <= atol, f"drone {i}: {dist.min(1).max()}"


@pytest.mark.parametrize("ntype", ["pos_vel_R", "pos"])
def test_reference_quiet_trajectory(golden, ntype):
    """The reference's noise-free 4-drone hover run with the type (traj_n4quiet_*.npz, 100 steps) replayed on the
    GPU, with the bounds of test_gpu_parity.py::test_reference_quiet_trajectory."""
    g = golden(f"traj_n4quiet_{ntype}")
    n, k, d = int(g["n"]), int(g["k"]), DIM[ntype]
    cfg = QuadSwarmConfig(num_envs=1, num_agents=n, neighbor_visible_num=k, neighbor_obs_type=ntype, sense_noise=None,
                          thrust_noise_ratio=0.0, episode_duration=15.0)
    assert cfg.obs_dim == g["obs"].shape[2] == 18 + d * k
    env = QuadSwarmEnv(cfg)
    env.reset()
    _load_initial_state(env, g, n)
    airborne = np.ones(n, bool)
    compared = 0
    for t in range(len(g["actions"])):
        obs, rew, done, _ = env.step(torch.from_numpy(g["actions"][t].astype(np.float32)).cuda())
        o = np_(obs)
        assert not done.any() and np.isfinite(o).all()
        want = g["obs"][t]
        airborne &= (want[:, 2] + 2.0) > 0.3
        m = airborne
        np.testing.assert_allclose(o[m, 0:3], want[m, 0:3], atol=2e-5 if t < 100 else 1e-4, err_msg=f"step {t}")
        np.testing.assert_allclose(o[m, :18], want[m, :18], atol=3e-4, err_msg=f"step {t}")
        np.testing.assert_allclose(np_(rew)[m], g["rew"][t][m], atol=2e-4, err_msg=f"step {t}")
        if m.all():
            _neighbors_close(o[:, 18:], want[:, 18:], d, atol=2e-2)
        compared += int(m.sum())
    assert compared >= n * 60


@pytest.mark.parametrize("ntype", ["pos", "pos_vel_R"])
def test_replay_runs_and_snapshots_carry_the_stale_rotation(ntype):
    """The reference's quad_multi_ablation shape (4 drones, mix, 3 visible neighbours, replay 0.75) for 60 steps:
    finite outputs.  The replay snapshots (qs_replay_buffers.snap_words) hold the stale rotation rows for the types
    that have them, and only for them: every checkpoint's 9 words per drone after the stale velocity are the
    live stale rotation.  A host snapshot restored into the env reproduces the next reset's obs bitwise."""
    cfg = QuadSwarmConfig(num_envs=128, num_agents=4, neighbor_visible_num=3, neighbor_obs_type=ntype, quads_mode="mix",
                          replay_buffer_sample_prob=0.75, episode_duration=1.0, seed=9)
    env = QuadSwarmEnv(cfg)
    assert env.replay is not None
    srows = 12 if ntype in ROT_TYPES else 3
    n = 4
    assert env.replay["snap_words"] == n * (N_.NF + N_.NI + srows + cfg.obs_dim) + N_.NE + N_.NENVF
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for t in range(60):
        a = (torch.rand(env.I, 4, device="cuda", generator=g) * 0.6 + 0.2).contiguous()
        obs, rew, done, term = env.step(a)
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert sum(env.counters().values()) == 0
    if ntype in ROT_TYPES:
        # checkpoints from the first episode on (the wrapper activates after hist_min history entries), every 5 ticks
        env = QuadSwarmEnv(QuadSwarmConfig(num_envs=128, num_agents=4, neighbor_visible_num=3, neighbor_obs_type=ntype,
                                           quads_mode="mix", episode_duration=1.0, seed=9))
        env.enable_replay(0.75, hist_min=1, cp_every=5)
        env.reset()
        for t in range(30):
            env.step((torch.rand(env.I, 4, device="cuda", generator=g) * 0.6 + 0.2).contiguous())
        store = env.replay["store"].cpu().numpy()
        off = n * (N_.NF + N_.NI + 3)
        rot = store[:, :, off:off + 9 * n].view(np.float32).reshape(128, -1, 9, n)
        used = store.any(axis=2)
        assert used.sum() >= 128 * 5
        R = np.moveaxis(rot, 2, 3)[used].reshape(-1, 3, 3).astype(np.float64)
        # inside the first episode the stale rotation is still what the first reset saw: the identity
        np.testing.assert_array_equal(R, np.broadcast_to(np.eye(3), R.shape))
        env.disable_replay()
        env.reset()              # QS_EF_STALE: the next reset reads the stale rows
        blob = env.get_state()
        o1 = env.reset().clone()
        env.stale_rot.fill_(0.5)
        env.stale_vel.fill_(0.25)
        env.set_state(blob)
        assert_same(env.reset(), o1, "reset obs after set_state")
