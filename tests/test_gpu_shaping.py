"""The reward shaping wrapper on the device (csrc/qs_shaping.h) against tests/shaping_restatement.py, the fp64
restatement of the reference's QuadsRewardShapingWrapper that tests/test_shaping_golden_cpu.py pins to fixtures
recorded from the reference's own wrapper.

Every case runs a twin handle without shaping on the same seed and actions: it supplies the uncorrected reward, and
everything the step writes must stay bitwise the twin's.  The restatement is driven by the GPU's own per-step rew_info,
done, actions and post-step scenario rows, one instance per env (rew_coeff is per multi-env)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from quadswarm_amd import QuadSwarmConfig  # noqa: E402
from quadswarm_amd import _native as N  # noqa: E402
from quadswarm_amd.env import QuadSwarmEnv  # noqa: E402
from quadswarm_amd.stats import SCENARIO_NAMES, shaping_infos  # noqa: E402
from quadswarm_amd.vec_env import GpuQuadVecEnv  # noqa: E402
from shaping_restatement import ShapingRestatement, make_scheme, reward_delta, step_rewards  # noqa: E402

SPACING = 0.08   # m between the drones of a written line: inside the collision hitbox 2 x arm = 0.0919 m (a line 0.1 m
                 # apart gives the proximity penalty only, so rew_info's QUADCOL row would stay 0)


def np_(t):
    return t.detach().cpu().numpy()


def make_cfg(E, n, k, c4=False, **over):
    kw = dict(num_envs=E, num_agents=n, seed=5, episode_duration=0.1, step_infos=True)
    kw.update(over)
    if c4:
        return QuadSwarmConfig.c4(**kw)
    return QuadSwarmConfig(neighbor_visible_num=k if k else 0, neighbor_obs_type="pos_vel" if k else "none", **kw)


def pair(cfg_fn, anneal=0.0, replay=None):
    """(env with shaping, twin without)."""
    env, twin = QuadSwarmEnv(cfg_fn()), QuadSwarmEnv(cfg_fn())
    if replay:
        env.enable_replay(**replay)
        twin.enable_replay(**replay)
    env.enable_reward_shaping(anneal)
    return env, twin


def scen_id(env, es, e):
    """QS_ES_SCEN's convention: the env row's mode word where the step keeps one, else 0 (static_same_goal)."""
    has = env.cfg.use_obstacles or env.cfg.quads_mode != "static_same_goal"
    return int(es[N.E_SC_MODE, e]) if has else 0


def scen_name(env, es, e):
    return "Scenario_" + SCENARIO_NAMES[scen_id(env, es, e)]


def poke_line(envs, rng, aim):
    """Write every env's drones onto a line SPACING apart at rest (identically in all handles); aim: the first three
    drones of every env head into a pillar instead, as tests/test_gpu_parity_obst.aim_at_obstacles does, from just
    outside its hit distance.  The previous-collision rows are cleared so every step's contacts count as new ones."""
    e0 = envs[0]
    E, n = e0.E, e0.N
    pos = np.zeros((E, n, 3), np.float32)
    vel = np.zeros((E, n, 3), np.float32)
    pos[:, :, 0] = -4.6 + SPACING * np.arange(n)[None, :]
    pos[:, :, 1] = -4.6
    pos[:, :, 2] = 2.0
    if aim:
        ob = np_(e0.obstacles)
        for e in range(E):
            for i in range(min(3, n)):
                o = ob[e, (i + e) % ob.shape[1]]
                ang = rng.uniform(-np.pi, np.pi)
                pos[e, i, :2] = o + 0.36 * np.array([np.cos(ang), np.sin(ang)])
                vel[e, i, :2] = -2.0 * np.array([np.cos(ang), np.sin(ang)])
    p = torch.from_numpy(pos.reshape(-1, 3).T.copy()).cuda()
    v = torch.from_numpy(vel.reshape(-1, 3).T.copy()).cuda()
    for env in envs:
        env.state[N.F_POS:N.F_POS + 3] = p
        env.state[N.F_VEL:N.F_VEL + 3] = v
        env.istate[N.I_PREV_LO:N.I_PREV_3 + 1] = 0
        env.istate[N.I_FLAGS] &= ~N.FL_PREV_OBST


BITWISE = ("obs", "rew", "done", "term_obs", "state", "istate", "env_state", "estats", "rew_info")


def assert_bitwise(env, twin, names, msg=""):
    for k in names:
        a, b = getattr(env, k), getattr(twin, k)
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                           b.view(torch.uint8) if b.dtype != torch.uint8 else b), f"{k} differs from the twin {msg}"


def run_case(env, twin, steps, anneal=0.0, s_of_t=None, mask_reset_after=None, poke=None, seed=0):
    """Step env + twin and the per-env restatements together; check every done row.  Returns a record."""
    cfg = env.cfg
    E, n, dt, obst = env.E, env.N, float(cfg.dt), cfg.use_obstacles
    # the handle's three collision coefficients (fp32 widened; quadcol_bin_obst is 0 without obstacles)
    fin = tuple(float(env.get_param(k)) for k in N.SH_COEF_NAMES)
    coeff = env.shaping_coefficients()
    rs, rcs = [], []
    for e in range(E):
        scheme, ann = make_scheme(fin[0], fin[1], fin[2], anneal)
        rc = dict(pos=1.0, effort=0.05, spin=0.1, vel=0.0, crash=1.0, orient=1.0, yaw=0.0,
                  quadcol_bin=0.0, quadcol_bin_smooth_max=0.0, quadcol_bin_obst=0.0)
        r = ShapingRestatement(n, rc, scheme, ann)
        r.reset()
        rs.append(r)
        rcs.append(rc)
    env.reset()
    twin.reset()
    rng = np.random.default_rng(seed)
    sums = np.zeros((N.NRI, env.I))
    ep_steps = np.zeros(E, dtype=np.int64)
    ends = np.zeros(E, dtype=np.int64)
    len_sum = np.zeros(E, dtype=np.int64)
    first_ep = np.ones(E, dtype=bool)
    reached = np.zeros(E, dtype=bool)
    rec = dict(quadcol_rows=0, prox_rows=0, obst_rows=0, bitwise_steps=0, corrected_steps=0, lens=[])
    S = 0.0
    sh = env.shaping
    for t in range(steps):
        if s_of_t is not None and t % 5 == 0:
            S = float(s_of_t(t))
            env.set_training_steps(S)
        if poke is not None:
            poke([env, twin], rng)
        a = rng.uniform(-1, 1, (env.I, 4)).astype(np.float32)
        at = torch.from_numpy(a).cuda()
        env.step(at)
        twin.step(at)
        torch.cuda.synchronize()
        comp = np_(env.rew_info)
        done = np_(env.done).astype(bool)
        rew, trew = np_(env.rew), np_(twin.rew)
        es = np_(env.env_state)
        row, coef, used = np_(sh["row"]), np_(sh["coef"]), np_(sh["coef_used"])
        assert_bitwise(env, twin, [k for k in BITWISE if k != "rew"], f"at step {t}")
        rec["quadcol_rows"] += int((comp[N.RI_QUADCOL] != 0).sum())
        rec["prox_rows"] += int((comp[N.RI_PROX] != 0).sum())
        rec["obst_rows"] += int((comp[N.RI_OBST] != 0).sum())
        sums += comp.astype(np.float64)
        ep_steps += 1
        for e in range(E):
            sl = slice(e * n, (e + 1) * n)
            c = rs[e].begin_step(a[sl].astype(np.float64))
            cu = np.array([c["quadcol_bin"], c["quadcol_bin_smooth_max"], c["quadcol_bin_obst"]])
            assert (np.abs(used[:, e] - cu) <= np.spacing(np.abs(cu))).all(), f"coef_used env {e} step {t}"
            # the reward: the twin's plus what the env's own coefficients change, rounded once to fp32
            want = (trew[sl].astype(np.float64) + reward_delta(comp[:, sl], c, fin)).astype(np.float32)
            bound = 2.0 ** -23 * np.maximum(np.abs(trew[sl]), np.abs(rew[sl]))
            assert (np.abs(rew[sl].astype(np.float64) - want) <= bound).all(), f"reward env {e} step {t}"
            if anneal > 0 and first_ep[e]:      # the first episode runs without the three swarm terms
                swarm = fin[0] * comp[N.RI_QUADCOL, sl] + comp[N.RI_PROX, sl].astype(np.float64) + fin[2] * comp[N.RI_OBST, sl]
                assert (np.abs(rew[sl] - (trew[sl] - swarm)) <= bound).all(), f"first episode env {e} step {t}"
            if (cu == np.array(fin)).all():
                assert (rew[sl].view(np.int32) == trew[sl].view(np.int32)).all(), f"env {e} step {t}: not the twin's bits"
                reached[e] = True
                rec["bitwise_steps"] += 1
            else:
                rec["corrected_steps"] += 1
            out = rs[e].end_step(step_rewards(comp[:, sl], c, fin[1], dt, obst), done[sl], scen_name(env, es, e), S)
            cn = np.array([rcs[e]["quadcol_bin"], rcs[e]["quadcol_bin_smooth_max"], rcs[e]["quadcol_bin_obst"]])
            assert (np.abs(coef[:, e] - cn) <= np.spacing(np.abs(cn))).all(), f"coef env {e} step {t}"
            if done[sl].any():
                assert done[sl].all()
                for i in range(n):
                    g = e * n + i
                    tr_w, st_w = out[i]
                    assert (row[g, N.SH_SUM:N.SH_SUM + N.NRI] == sums[:, g]).all(), f"raw sums drone {g} step {t}"
                    assert row[g, N.SH_LEN] == ep_steps[e] and row[g, N.SH_SCEN] == scen_id(env, es, e)
                    tr, st = shaping_infos(row[g], coeff, dt, obst, annealing=anneal > 0)
                    assert sorted(st) == sorted(st_w)
                    np.testing.assert_allclose(tr, tr_w, rtol=1e-12, atol=0)
                    np.testing.assert_allclose(row[g, N.SH_TRUE_REWARD], tr_w, rtol=1e-12, atol=0)
                    for k in st_w:
                        if k.startswith("z_action"):
                            atol = 1e-13 if k.endswith("_mean") else 1e-10
                            assert abs(st[k] - st_w[k]) <= atol, (k, st[k], st_w[k])
                        else:
                            np.testing.assert_allclose(st[k], st_w[k], rtol=1e-12, atol=0, err_msg=f"{k} drone {g} step {t}")
                sums[:, sl] = 0
                len_sum[e] += ep_steps[e]
                rec["lens"].append(int(ep_steps[e]))
                ep_steps[e] = 0
                ends[e] += 1
                first_ep[e] = False
        if mask_reset_after is not None and t == mask_reset_after:
            m = np.zeros(E, np.uint8)
            m[1] = 1
            env.reset(m)
            twin.reset(m)
            rs[1].reset()
            sums[:, n:2 * n] = 0
            ep_steps[1] = 0
    rec.update(ends=ends, reached=reached, len_sum=len_sum)
    return rec


CASES = [(5, 3, 2, False), (4, 8, 6, False), (3, 1, 0, False), (2, 128, 6, False), (4, 8, 2, True)]


@pytest.mark.parametrize("E,n,k,c4", CASES, ids=["5x3", "4x8", "3x1", "2x128", "c4"])
def test_sums(E, n, k, c4):
    env, twin = pair(lambda: make_cfg(E, n, k, c4))
    rec = run_case(env, twin, 35, mask_reset_after=4)
    print("sums", (E, n, k, c4), rec)
    assert (rec["ends"] >= 2).all(), rec["ends"]
    torch.cuda.synchronize()
    assert_bitwise(env, twin, BITWISE, "after the last step")   # no annealing: rew too
    tot_n, tot = np_(env.shaping["tot_n"]), np_(env.shaping["tot"])
    E_, n_ = env.E, env.N
    assert (tot_n.reshape(E_, n_) == rec["ends"][:, None]).all()
    assert (tot[:, N.SH_LEN].reshape(E_, n_) == rec["len_sum"][:, None]).all()
    env.close()
    twin.close()


def test_constant_actions():
    env = QuadSwarmEnv(make_cfg(3, 8, 6))
    env.enable_reward_shaping()
    env.reset()
    a = torch.full((env.I, 4), 0.25, device="cuda")
    for _ in range(11):
        env.step(a)
    torch.cuda.synchronize()
    assert (np_(env.shaping["tot_n"]) == 1).all()
    row = np_(env.shaping["row"])
    std, mean = row[:, N.SH_ACT_STD:N.SH_ACT_STD + 4], row[:, N.SH_ACT_MEAN:N.SH_ACT_MEAN + 4]
    assert np.isfinite(std).all() and (std >= 0).all() and (std <= 1e-5).all(), std.max()
    assert (mean == 0.25).all()
    env.close()


@pytest.mark.parametrize("c4", [False, True], ids=["4x8", "c4"])
def test_annealing(c4):
    steps, anneal = 60, 2000.0
    env, twin = pair(lambda: make_cfg(4, 8, 6 if not c4 else 2, c4), anneal=anneal)
    # S passes anneal_steps about two thirds through
    rec = run_case(env, twin, steps, anneal=anneal, s_of_t=lambda t: 50.0 * t,
                   poke=lambda envs, rng: poke_line(envs, rng, aim=c4))
    n = env.N
    print("annealing", "c4" if c4 else "4x8", rec)
    assert rec["quadcol_rows"] >= n and rec["prox_rows"] >= n, rec
    if c4:
        assert rec["obst_rows"] >= 1, rec
    assert rec["reached"].all() and rec["corrected_steps"] > 0 and rec["bitwise_steps"] > 0, rec
    assert (rec["ends"] >= 4).all()
    env.close()
    twin.close()


def test_vec_env_rewards_use_the_envs_coefficient():
    cfg = make_cfg(3, 4, 3, reward_shaping=True, anneal_collision_steps=1000.0)
    venv = GpuQuadVecEnv(cfg)
    venv.reset()
    rng = np.random.default_rng(1)
    seen = set()
    finished = 0
    for t in range(34):
        venv.env.set_training_steps(40.0 * t)
        poke_line([venv.env], rng, aim=False)
        _, _, dones, infos = venv.step(rng.uniform(-1, 1, (venv.num_envs, 4)).astype(np.float32))
        used, comp = np_(venv.env.shaping["coef_used"]), np_(venv.env.rew_info)
        for i in range(venv.num_envs):
            e = i // 4
            assert infos[i]["rewards"]["rew_quadcol"] == used[0, e] * float(comp[N.RI_QUADCOL, i])
            if comp[N.RI_QUADCOL, i] != 0:
                seen.add(float(used[0, e]))
            if dones[i]:
                finished += 1
                st = infos[i]["episode_extra_stats"]
                assert infos[i]["true_reward"] == st["rewraw_main"]
                assert {"z_anneal_quadcol_bin", "z_action0_mean", "rew_quadcol", "z_approx_total_training_steps"} <= set(st)
                assert "num_collisions" in st or "num_collisions_replay" in st   # the env's own stats are still there
    assert finished >= 3 * 4 * 2 and len(seen) >= 3, (finished, seen)   # 0, intermediate values, the final 5.0
    venv.close()


def test_replay_on():
    """Replay restores put an env back in the middle of an earlier episode: the wrapper's episode (its sums, its step
    count) still runs from the restore to the next done, and the scenario the row names is the restored one.  The
    replay rules run at a short time scale and a line of drones is written every 4th step (into the twin too) so
    that collision events, and with them replays, happen within 150 steps."""
    E, n = 8, 8
    mk = lambda: make_cfg(E, n, 6, quads_mode="mix")   # noqa: E731
    rp = dict(sample_prob=0.75, cp_every=2, grace_ticks=2, min_gap_ticks=3, hist_min=1, steps_ago=1)
    env, twin = pair(mk, replay=rp)
    calls = [0]

    def poke(envs, rng):
        calls[0] += 1
        if calls[0] % 4 == 0:
            poke_line(envs, rng, aim=False)
    rec = run_case(env, twin, 150, poke=poke, seed=3)
    replayed = np_(env.replay["ri"])[N.R_REPLAYED]
    print("replay", rec, replayed)
    assert (rec["ends"] >= 2).all()
    assert replayed.sum() >= E, "too few replayed episodes for the case to mean anything"
    full = int(env.get_param("ep_len")) + 1
    assert max(rec["lens"]) == full and min(rec["lens"]) < full, "a restore shortened at least one recorded episode"
    # run_case compared each row's scenario id with env_state[E_SC_MODE] read after the same step
    assert len(set(np_(env.shaping["row"])[:, N.SH_SCEN].tolist())) > 1, "mix: more than one scenario was recorded"
    env.close()
    twin.close()


def workspace(env):
    torch.cuda.synchronize()
    return env._shaping_ws.clone()


def drive(env, steps, seed=0):
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in range(steps):
        a = torch.rand((env.I, 4), device="cuda", generator=g) * 2 - 1
        if t % 5 == 0:
            env.set_training_steps(30.0 * t)
        env.step(a)
    return workspace(env)


def test_deterministic():
    ws = []
    for _ in range(2):
        env = QuadSwarmEnv(make_cfg(4, 8, 6))
        env.enable_reward_shaping(500.0)
        ws.append(drive(env, 35))
        env.close()
    assert torch.equal(ws[0], ws[1])


def test_shards():
    """One E = 6 handle against two E = 3 shards with drone_id_offset: an env's rows depend on the env alone."""
    n = 8
    full = QuadSwarmEnv(make_cfg(6, n, 6))
    parts = [QuadSwarmEnv(make_cfg(3, n, 6, drone_id_offset=3 * n * s)) for s in range(2)]
    for e in [full] + parts:
        e.enable_reward_shaping(500.0)
        e.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for t in range(35):
        a = torch.rand((full.I, 4), device="cuda", generator=g) * 2 - 1
        for e in [full] + parts:
            if t % 5 == 0:
                e.set_training_steps(30.0 * t)
        full.step(a)
        for s, p in enumerate(parts):
            p.step(a[s * p.I:(s + 1) * p.I].contiguous())
    torch.cuda.synchronize()
    assert (full.shaping["tot_n"] >= 3).all()
    for k in ("row", "tot", "tot_n", "acc"):
        cat = torch.cat([p.shaping[k] for p in parts], dim=1 if k == "acc" else 0)
        assert torch.equal(full.shaping[k], cat), k
    for e in [full] + parts:
        e.close()


def test_graph():
    """env.step captured with torch.cuda.graph on one stream holds the shaping kernel: 25 replays with new actions
    and set_training_steps between them give bitwise the workspace of 25 eager steps."""
    def run(graph):
        env = QuadSwarmEnv(make_cfg(4, 8, 6))
        env.enable_reward_shaping(500.0)
        env.reset()
        g = torch.Generator(device="cuda").manual_seed(7)
        a = torch.zeros((env.I, 4), device="cuda")
        gr = None
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            ws0 = workspace(env)
            st0 = env.get_state()
            with torch.cuda.stream(s):
                env.step(a)                      # warm-up on the capture stream
            torch.cuda.synchronize()
            env.set_state(st0)                   # undo the warm-up step
            env._shaping_ws.copy_(ws0)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                env.step(a)
        for t in range(25):
            a.copy_(torch.rand((env.I, 4), device="cuda", generator=g) * 2 - 1)
            if t % 5 == 0:
                env.set_training_steps(30.0 * t)
            if graph:
                gr.replay()
            else:
                env.step(a)
        out = workspace(env), env.rew.clone(), env.obs.clone()
        assert (env.shaping["tot_n"] >= 2).all()
        env.close()
        return out
    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals():
    import ctypes
    L = N.lib()
    a = QuadSwarmEnv(QuadSwarmConfig.sb_train(num_envs=2, num_agents=4))
    sc = N.QsShapingConfig()
    nb = ctypes.c_size_t()
    assert L.qs_shaping_workspace_bytes(a._h, ctypes.byref(sc), ctypes.byref(nb)) == -2      # QS_E_UNSUPPORTED
    assert b"flavor" in L.qs_last_error()
    with pytest.raises(N.QuadSwarmError):
        a.enable_reward_shaping()
    a.close()
    b = QuadSwarmEnv(QuadSwarmConfig(num_envs=2, num_agents=4, neighbor_visible_num=3))      # step_infos off
    assert L.qs_shaping_workspace_bytes(b._h, ctypes.byref(sc), ctypes.byref(nb)) == -1      # QS_E_INVALID
    with pytest.raises(N.QuadSwarmError):
        b.set_training_steps(1.0)
    b.close()
    c = QuadSwarmEnv(make_cfg(2, 4, 3))
    c.enable_reward_shaping()
    c.reset()
    c.disable_reward_shaping()
    assert c.shaping is None
    c.step(torch.zeros((c.I, 4), device="cuda"))
    torch.cuda.synchronize()
    c.close()


def test_trainer_episode_records(tmp_path):
    """PPOTrainer with the wrapper on: the clock reaches the device before each rollout, the records are the finished
    episodes' means (checked against the rows on the host), and the workspace travels in a checkpoint."""
    from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic
    cfg = make_cfg(8, 8, 6, reward_shaping=True, anneal_collision_steps=5000.0)
    env = QuadSwarmEnv(cfg)
    pol = SwarmActorCritic(PolicyConfig.for_env(cfg, rnn_size=64, neighbor_hidden_size=64)).cuda()
    tr = PPOTrainer(env, pol, PPOConfig(n_steps=24, batch_size=512, n_epochs=1), seed=1)
    tr.collect_rollouts()
    r = dict(tr.episode_records)
    torch.cuda.synchronize()
    assert float(env.shaping["S"][0]) == 0.0
    tot, tot_n = np_(env.shaping["tot"]), np_(env.shaping["tot_n"])
    ep = int(env.get_param("ep_len")) + 1                             # done when tick > ep_len
    k = 24 // ep
    assert k >= 2 and r["rollout/episodes"] == tot_n.sum() == k * env.I
    np.testing.assert_allclose(r["rollout/ep_true_reward_mean"], tot[:, N.SH_TRUE_REWARD].sum() / tot_n.sum(), rtol=1e-12)
    assert r["rollout/ep_len_mean"] == float(ep)
    # SB3's ep_rew_mean: the summed step rewards (fp32 each, so 1e-5 relative on their mean); the rollout's rewards
    # cover k whole episodes and a few more steps
    rew_sum = tr.storage.rewards[:k * ep].double().sum().item() / (k * env.I)
    np.testing.assert_allclose(r["rollout/ep_rew_mean"], rew_sum, rtol=1e-5)
    tr.train(max_updates=1)
    path = tr.save(str(tmp_path / "ck.pt"))
    tr.collect_rollouts()
    assert float(env.shaping["S"][0]) == 24 * env.I
    want = (dict(tr.episode_records), workspace(env))
    tr.load(path)
    tr.collect_rollouts()
    assert tr.episode_records == want[0] and torch.equal(workspace(env), want[1])
    # a callback that stops the rollout early: the episodes of the partial rollout are still reported
    from quadswarm_amd.callbacks import TrainerCallback

    class Stop(TrainerCallback):
        def on_step(self, ctx):
            return ctx.t < ep + 1

    before = int(np_(env.shaping["tot_n"]).sum())
    assert tr.collect_rollouts([Stop()]) is False
    torch.cuda.synchronize()
    ended = int(np_(env.shaping["tot_n"]).sum()) - before
    assert ended >= env.I and tr.episode_records["rollout/episodes"] == ended
    env.close()


@pytest.mark.parametrize("mode,obst,want", [("o_random", True, 16), ("o_static_same_goal", True, 17),
                                            ("o_swap_goals", True, 19), ("swap_goals", False, 7),
                                            ("static_same_goal", False, 0)])
def test_scenario_id_of_a_fixed_scenario(mode, obst, want):
    """The row's scenario id against the id the configured scenario has by definition (quadswarm_amd.stats.
    SCENARIO_NAMES), not against the env word the kernel reads.  With obstacles the config asks for reward shaping
    with episode_stats off: to_qs_config turns the stats on, since the kernels keep that word with them."""
    from quadswarm_amd.stats import SCENARIO_NAMES as NAMES
    assert NAMES[want] == mode
    cfg = make_cfg(3, 4, 2, c4=obst, quads_mode=mode, reward_shaping=True, episode_stats=False)
    assert cfg.to_qs_config().episode_stats == (1 if obst else 0)
    env = QuadSwarmEnv(cfg)
    env.reset()
    a = torch.zeros((env.I, 4), device="cuda")
    for _ in range(12):
        env.step(a)
    torch.cuda.synchronize()
    assert (np_(env.shaping["tot_n"]) == 1).all()
    row = np_(env.shaping["row"])
    assert (row[:, N.SH_SCEN] == want).all(), row[:, N.SH_SCEN]
    _, st = shaping_infos(row[0], env.shaping_coefficients(), float(cfg.dt), obst)
    assert f"Scenario_{mode}/rew_pos" in st
    env.close()


def test_obstacles_without_episode_stats_are_refused():
    import ctypes
    cfg = make_cfg(2, 4, 2, c4=True, episode_stats=False)      # shaping not configured: the stats stay off
    env = QuadSwarmEnv(cfg)
    sc, nb = N.QsShapingConfig(), ctypes.c_size_t()
    assert N.lib().qs_shaping_workspace_bytes(env._h, ctypes.byref(sc), ctypes.byref(nb)) == -1     # QS_E_INVALID
    assert b"episode_stats" in N.lib().qs_last_error()
    with pytest.raises(N.QuadSwarmError, match="episode_stats"):
        env.enable_reward_shaping()
    assert env.shaping is None
    env.close()


def test_vec_env_native_mode():
    """as_torch=True: nothing is read in step_wait; resolve() builds every row's rewards with the env's coefficient of
    that step and finished rows carry true_reward and the merged stats."""
    cfg = make_cfg(3, 4, 3, reward_shaping=True, anneal_collision_steps=1000.0)
    venv = GpuQuadVecEnv(cfg, as_torch=True)
    venv.reset()
    rng = np.random.default_rng(1)
    g = torch.Generator(device="cuda").manual_seed(3)
    seen, finished = set(), 0
    for t in range(34):
        venv.env.set_training_steps(40.0 * t)
        poke_line([venv.env], rng, aim=False)
        a = torch.rand((venv.num_envs, 4), device="cuda", generator=g) * 2 - 1
        if t > 0:                                        # the first step warms the allocator up
            torch.cuda.set_sync_debug_mode("error")      # a host sync inside step_wait raises
        try:
            _, _, dones, infos = venv.step(a)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        used, comp, d = np_(venv.env.shaping["coef_used"]), np_(venv.env.rew_info), np_(dones)
        for i in range(venv.num_envs):
            e = i // 4
            assert infos[i]["rewards"]["rew_quadcol"] == used[0, e] * float(comp[N.RI_QUADCOL, i])
            if comp[N.RI_QUADCOL, i] != 0:
                seen.add(float(used[0, e]))
            if d[i]:
                finished += 1
                st = infos[i]["episode_extra_stats"]
                assert infos[i]["true_reward"] == st["rewraw_main"]
                assert {"z_anneal_quadcol_bin", "z_action0_mean", "rew_quadcol", "num_collisions"} <= set(st)
            else:
                assert "true_reward" not in infos[i]
    assert finished >= 3 * 4 * 2 and len(seen) >= 3, (finished, seen)
    venv.close()
