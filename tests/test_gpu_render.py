"""qs_render on the device against the fp64 numpy restatement (tests/render_restatement.py).

The state is read back from the env's own tensors and restated; outside the edge band (tests/test_render_cpu.py:
4 x the measured fp32 / fp64 displacement) every pixel is equal, and the banded pixels are at most 1 % of a frame.
The shapes are the smallest at which the kernel can still go wrong: partial tiles, several tiles, several envs, more
than 1024 primitives, inactive pillar slots, repeated env ids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from quadswarm_amd import QuadSwarmConfig, _native as N  # noqa: E402
from quadswarm_amd.render import (PAL_BORDER, PAL_INSIDE, PAL_OBSTACLE, PAL_OUTSIDE, PAL_TARGET, PALETTE,  # noqa: E402
                                  RenderConfig, tile_images)
from render_restatement import restate  # noqa: E402
from test_render_cpu import CAP, band  # noqa: E402

DEV = "cuda:0"


def _env(cfg):
    from quadswarm_amd.env import QuadSwarmEnv
    cfg.specialize = False           # the renderer reads the state; which step kernels wrote it does not matter
    return QuadSwarmEnv(cfg, device=DEV)


def _random_steps(env, steps, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(steps):
        env.step((torch.rand(env.I, env.act_dim, generator=g) * 2 - 1).to(DEV))


def scene_of(env, e):
    """env e of the device state as a restatement scene"""
    n, q = env.N, env.qcfg
    sl = slice(e * n, (e + 1) * n)
    st = env.state[:, sl].double().cpu().numpy()
    sc = dict(pos=st[N.F_POS:N.F_POS + 3].T, rot=st[N.F_ROT:N.F_ROT + 9].T.reshape(n, 3, 3), goal=st[N.F_GOAL:N.F_GOAL + 3].T,
              on_floor=(env.istate[N.I_FLAGS, sl].cpu().numpy() & N.FL_ON_FLOOR) != 0,
              room_lo=np.array(list(q.room_lo), dtype=np.float32), room_hi=np.array(list(q.room_hi), dtype=np.float32),
              arm=np.float32(q.arm), flavor=env.cfg.flavor)
    if env.cfg.flavor == "A":
        ef = env.env_f[:, e].double().cpu().numpy()
        sc["target"] = np.array([ef[N.ENVF_TARGET_X], ef[N.ENVF_TARGET_Y], 2.0])   # dynamic_repulsive.py: the target's height
        sc["capture"] = ef[N.ENVF_CAPTURE]
    if env.obstacles is not None:
        es = env.env_state[:, e].cpu().numpy()
        mi, si = int(es[N.E_OBST_M]), int(es[N.E_OBST_SZ])      # 0 = configured, c + 1 = the c-th table entry
        count = q.num_obstacles if mi == 0 else q.dr_counts[mi - 1]
        sc["obst_size"] = np.float32(q.obst_size if si == 0 else q.dr_sizes[si - 1])
        sc["obst"] = env.obstacles[e, :count].double().cpu().numpy()
    return sc


def check(env, ids, rc, frames=None):
    if frames is None:
        frames = env.render(ids, rc)
    assert frames.dtype == env._torch.uint8 and tuple(frames.shape) == (len(ids), rc.height, rc.width, 3)
    assert frames.device == env.device
    got = frames.cpu().numpy()
    for k, e in enumerate(ids):
        want, edge, _ = restate(scene_of(env, e), rc.width, rc.height, view=rc.view, follow=rc.follow,
                                drone_scale=rc.drone_scale, dtype=np.float64)
        banded = edge <= band()
        bad = (got[k] != want).any(-1) & ~banded
        print(f"env {e}: {int(banded.sum())} of {banded.size} pixels in the band, {int(bad.sum())} differ outside it")
        assert banded.mean() <= CAP
        assert not bad.any(), np.argwhere(bad)[:8]
    return got


def has(frame, k):
    return bool((frame.reshape(-1, 3) == PALETTE[k]).all(1).any())


@pytest.fixture(scope="module")
def b8():
    env = _env(QuadSwarmConfig(num_envs=4, num_agents=8, seed=11))
    env.reset()
    yield env
    env.close()


def test_b8_topdown_after_reset(b8):
    b8.reset()
    got = check(b8, [0, 1, 2, 3], RenderConfig(width=64, height=48, view="topdown"))
    assert all(has(got[0], k) for k in (PAL_OUTSIDE, PAL_INSIDE, PAL_BORDER)) and any(has(got[0], i) for i in range(8))


def test_b8_partial_tiles_order_and_repeats(b8):
    """68 x 50: two tile columns (64 + 4 pixels) and four tile rows (the last of 2 rows); env ids [3, 0, 3]"""
    b8.reset()
    _random_steps(b8, 3, seed=2)
    got = check(b8, [3, 0, 3], RenderConfig(width=68, height=50, view="topdown", drone_scale=4.0))
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])


def test_b8_follow_side_and_front():
    env = _env(QuadSwarmConfig(num_envs=2, num_agents=8, seed=5))
    env.reset()
    _random_steps(env, 5, seed=1)
    for view in ("side", "front"):
        check(env, [0, 1], RenderConfig(width=96, height=64, view=view, follow=True, drone_scale=4.0))
    env.close()


def test_c4_obstacles_inactive_slots_are_not_drawn():
    cfg = QuadSwarmConfig.c4(num_envs=4, seed=3, replay_buffer_sample_prob=0.75, domain_random=True,
                             obst_density_random=True)
    env = _env(cfg)
    env.reset()
    counts = cfg.domain_random_tables()[1]
    assert min(counts) < cfg.max_obstacles == env.obstacles.shape[1]
    env.env_state[N.E_OBST_M, 1] = 1 + counts.index(min(counts))     # env 1: the smallest pillar count of the table
    for view in ("topdown", "side"):
        got = check(env, [0, 1, 2, 3], RenderConfig(width=128, height=128, view=view))
        assert has(got[1], PAL_OBSTACLE)
    # fewer pillars, fewer pillar pixels than the same env drawn with every slot active
    few = (env.render([1], RenderConfig(width=128, height=128)).cpu().numpy() == PALETTE[PAL_OBSTACLE]).all(-1).sum()
    env.env_state[N.E_OBST_M, 1] = 1 + counts.index(max(counts))
    many = (env.render([1], RenderConfig(width=128, height=128)).cpu().numpy() == PALETTE[PAL_OBSTACLE]).all(-1).sum()
    assert 0 < few < many
    env.close()


def test_a4_target_cross_and_capture_ring_follow_the_radius():
    env = _env(QuadSwarmConfig.sb_train(num_envs=2, num_agents=4, seed=7))
    env.reset()
    _random_steps(env, 2)
    rc = RenderConfig(width=96, height=96, view="topdown")
    wide = check(env, [0, 1], rc)
    env.set_capture_radius(1.1)
    narrow = check(env, [0, 1], rc)
    env.set_capture_radius(0.6, env_indices=[1])
    one = check(env, [0, 1], rc)
    assert has(wide[0], PAL_TARGET) and not np.array_equal(wide[0], narrow[0])
    assert np.array_equal(one[0], narrow[0]) and not np.array_equal(one[1], narrow[1])
    env.close()


@pytest.fixture(scope="module")
def n128():
    env = _env(QuadSwarmConfig(num_envs=2, num_agents=128, neighbor_visible_num=6, seed=2))
    env.reset()
    _random_steps(env, 3)
    yield env
    env.close()


def test_n128_follow_chunked_cull(n128):
    """128 drones: 1280 primitives, so each wave's cull runs 20 passes of 64"""
    check(n128, [1, 0], RenderConfig(width=128, height=96, view="topdown", follow=True))


def test_determinism(n128):
    rc = RenderConfig(width=128, height=96, view="topdown", follow=True)
    a = torch.zeros(2, 96, 128, 3, dtype=torch.uint8, device=DEV)
    b = torch.full((2, 96, 128, 3), 255, dtype=torch.uint8, device=DEV)
    assert n128.render([0, 1], rc, out=a) is a
    n128.render([0, 1], rc, out=b)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        n128.render([0, 2], rc)                              # env ids are checked on the host list
    with pytest.raises(ValueError):
        n128.render([0], rc, out=a)                          # a buffer of another shape


def test_hand_made_frame():
    """One drone at the centre of a 10 x 8 m floor, identity rotation, topdown 64 x 64: s = 5.6 px/m, the room spans
    columns 4 .. 60 and rows 9.6 .. 54.4, the drone's body (0.75 px) covers the four pixels around (32, 32)."""
    env = _env(QuadSwarmConfig(num_envs=1, num_agents=1, neighbor_obs_type="none", neighbor_visible_num=0,
                               room_dims=(10.0, 8.0, 10.0)))
    env.reset()
    env.state[N.F_POS:N.F_POS + 3, 0] = torch.tensor([0.0, 0.0, 5.0], device=DEV)
    env.state[N.F_GOAL:N.F_GOAL + 3, 0] = torch.tensor([0.0, 0.0, 5.0], device=DEV)
    env.state[N.F_ROT:N.F_ROT + 9, 0] = torch.eye(3, device=DEV).reshape(9)
    env.istate[N.I_FLAGS, 0] = 0
    f = env.render(cfg=RenderConfig(width=64, height=64)).cpu().numpy()[0]
    assert tuple(f[32, 32]) == tuple(PALETTE[0]) and tuple(f[31, 31]) == tuple(PALETTE[0])
    assert tuple(f[32, 42]) == tuple(PALETTE[PAL_INSIDE]) and tuple(f[22, 32]) == tuple(PALETTE[PAL_INSIDE])
    assert tuple(f[0, 0]) == tuple(PALETTE[PAL_OUTSIDE]) and tuple(f[7, 32]) == tuple(PALETTE[PAL_OUTSIDE])
    assert tuple(f[9, 32]) == tuple(PALETTE[PAL_BORDER]) and tuple(f[54, 20]) == tuple(PALETTE[PAL_BORDER])
    assert tuple(f[30, 32]) == tuple(PALETTE[0])            # the goal ring (1.5 .. 2.5 px) in the drone's colour
    env.istate[N.I_FLAGS, 0] = N.FL_ON_FLOOR
    f = env.render(cfg=RenderConfig(width=64, height=64)).cpu().numpy()[0]
    assert tuple(f[32, 32]) == tuple(PALETTE[16])           # on the floor: half intensity
    env.close()


def test_render_is_read_only():
    envs = [_env(QuadSwarmConfig(num_envs=4, num_agents=8, seed=9)) for _ in range(2)]
    for env in envs:
        env.reset()
    before = envs[0].get_state()
    rc = RenderConfig(width=64, height=48, follow=True)
    buf = envs[0].render([0, 1, 2, 3], rc)
    assert envs[0].get_state() == before
    g = torch.Generator(device="cpu").manual_seed(4)
    for _ in range(8):
        a = (torch.rand(envs[0].I, 4, generator=g) * 2 - 1).to(DEV)
        outs = [[t.clone() for t in env.step(a)[:3]] for env in envs]
        envs[0].render([0, 1, 2, 3], rc, out=buf)          # the twin never renders
        for x, y in zip(*outs):
            assert torch.equal(x, y)
    assert envs[0].get_state() == envs[1].get_state()
    for env in envs:
        env.close()


def test_render_orders_after_the_step_on_its_stream(b8):
    b8.reset()
    rc = RenderConfig(width=96, height=64, view="side")
    before = b8.render([0, 1], rc).clone()
    a = -torch.ones(b8.I, 4, device=DEV)                    # motors off: half a second of free fall
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        b8.step_n(a, 50)
        f1 = b8.render([0, 1], rc)                           # no synchronisation between the steps and the render
    torch.cuda.synchronize()
    f2 = b8.render([0, 1], rc)
    assert torch.equal(f1, f2) and not torch.equal(f1, before)
    check(b8, [0, 1], rc, frames=f1)


def test_vec_env_surface():
    from quadswarm_amd.vec_env import GpuQuadVecEnv
    rc = RenderConfig(width=64, height=48)
    v = GpuQuadVecEnv(QuadSwarmConfig(num_envs=4, num_agents=8, specialize=False), device=DEV, render_mode="rgb_array",
                      render_envs=(0, 1, 2), render_config=rc)
    v.reset()
    img = v.render()
    want = tile_images(np.zeros((3, 48, 64, 3), np.uint8))
    assert isinstance(img, np.ndarray) and img.shape == want.shape == (96, 128, 3) and img.dtype == np.uint8
    ims = v.get_images()
    assert len(ims) == 3 and all(i.shape == (48, 64, 3) and i.dtype == np.uint8 for i in ims)
    assert np.array_equal(img, tile_images(ims)) and v.render(mode="rgb_array").shape == want.shape
    assert np.array_equal(ims[1], v.env.render([1], rc).cpu().numpy()[0])
    v.close()
    d = GpuQuadVecEnv(QuadSwarmConfig(num_envs=2, num_agents=8, specialize=False), device=DEV)
    d.reset()
    assert d.render_mode is None and d.render() is None
    d.close()
    with pytest.raises(ValueError):
        GpuQuadVecEnv(QuadSwarmConfig(num_envs=2, num_agents=8, specialize=False), device=DEV, render_mode="human")
