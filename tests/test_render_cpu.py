"""CPU-side checks of the headless renderer: qs_render_query's validation, the palette mirror, the host helpers, and
the numpy restatement (tests/render_restatement.py) that the GPU tests compare the kernel with.

Edge band.  A frame is reproducible up to the pixels whose centre sits on a primitive's edge; a comparison between two
arithmetics leaves out the pixels nearer than BAND to any edge.  BAND is not chosen: it is 4 x the largest
displacement, in pixels, of any primitive centre, end point, radius or bound between the restatement in fp32 and in
fp64, measured on the scenes below (the factor covers what the kernel does differently from numpy's fp32: operation
order, fma contraction, the hardware's division).
    measured displacement: 8.37e-06 px (scene n128_follow)  ->  BAND = 3.35e-05 px
Cap (a condition, not a measurement): the banded pixels are at most 1 % of a frame, for every scene.
"""
import ctypes
import functools
import os
import re
import struct
import zlib

import numpy as np
import pytest

from quadswarm_amd import QuadSwarmConfig, _native as N
from quadswarm_amd.render import PALETTE, RenderConfig, tile_images, write_png
from render_restatement import displacement, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARM = 0.04596194077712559
DOCUMENTED_DISPLACEMENT = 8.37e-06     # the module docstring's figure
CAP = 0.01


# ---------------------------------------------------------------------------------------------------------------
# scenes: synthetic, from numpy seeds; the shapes are the GPU tests' (tests/test_gpu_render.py)
# ---------------------------------------------------------------------------------------------------------------
def _rotations(rng, n, tilt=0.6):
    """yawed and tilted body -> world rotations: Rz(yaw) Ry(pitch) Rx(roll)"""
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi, n), rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n)
    out = np.zeros((n, 3, 3))
    for i in range(n):
        cy, sy, cp, sp, cr, sr = np.cos(yaw[i]), np.sin(yaw[i]), np.cos(pitch[i]), np.sin(pitch[i]), np.cos(roll[i]), np.sin(roll[i])
        rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
        ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
        rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        out[i] = rz @ ry @ rx
    return out


def _swarm(seed, n, room=(10.0, 10.0, 10.0), box=2.0, flavor="B"):
    rng = np.random.default_rng(seed)
    lo = np.array([-room[0] / 2, -room[1] / 2, 0.0])
    hi = np.array([room[0] / 2, room[1] / 2, room[2]])
    pos = np.column_stack([rng.uniform(-box, box, n), rng.uniform(-box, box, n), rng.uniform(0.3, min(3.0, room[2]), n)])
    sc = dict(pos=pos, rot=_rotations(rng, n), goal=pos + rng.normal(0, 0.4, (n, 3)), on_floor=np.zeros(n, bool),
              room_lo=lo, room_hi=hi, arm=ARM, flavor=flavor)
    sc["on_floor"][1 % n] = True                      # one drone on the floor
    sc["pos"][1 % n, 2] = ARM
    if n > 3:
        sc["pos"][3] = sc["pos"][2] + [0.03, -0.02, 0.01]   # two overlapping drones
    return sc, rng


@functools.lru_cache(maxsize=None)
def scenes():
    out = []
    s, _ = _swarm(1, 8)
    s["goal"] = s["pos"].copy()                       # right after a reset: goals on top of the drones
    out.append(("b8_reset", s, 64, 48, dict(view="topdown")))
    s, _ = _swarm(2, 8)
    s["pos"][7] = [3.9, -3.3, 6.1]                    # one drone far from the rest: it sets the follow window
    out.append(("b8_follow_side", s, 96, 64, dict(view="side", follow=True, drone_scale=4.0)))
    out.append(("b8_follow_front", s, 96, 64, dict(view="front", follow=True, drone_scale=4.0)))
    s, rng = _swarm(3, 8)
    cells = rng.permutation(64)[:7]                   # 7 active pillars on the 8 x 8 grid of 1 m cells
    s["obst"] = np.column_stack([cells % 8 - 3.5, cells // 8 - 3.5]) + rng.uniform(-0.2, 0.2, (7, 2))
    s["obst_size"] = 0.6
    out.append(("c4_topdown", s, 128, 128, dict(view="topdown")))
    out.append(("c4_side", s, 128, 128, dict(view="side")))
    s, rng = _swarm(4, 4, room=(15.0, 15.0, 3.0), box=5.0, flavor="A")
    s["target"] = np.array([1.37, -2.21, 2.0])
    s["capture"] = 1.3
    out.append(("a4_target", s, 96, 96, dict(view="topdown")))
    s, _ = _swarm(5, 128, box=3.0)
    out.append(("n128_follow", s, 128, 96, dict(view="topdown", follow=True)))
    s, _ = _swarm(6, 8)
    out.append(("b8_partial_tiles", s, 68, 50, dict(view="topdown")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def measured_displacement():
    return max((displacement(s, w, h, **kw), name) for name, s, w, h, kw in scenes())


def band():
    """the comparison band in pixels: 4 x the measured fp32 / fp64 displacement (module docstring)"""
    return 4.0 * measured_displacement()[0]


@functools.lru_cache(maxsize=None)
def _restated(i, dtype):
    name, s, w, h, kw = scenes()[i]
    return restate(s, w, h, dtype=dtype, **kw)


# ---------------------------------------------------------------------------------------------------------------
def _configs():
    return {"c3": QuadSwarmConfig(num_envs=4, num_agents=8), "c4": QuadSwarmConfig.c4(num_envs=4),
            "sb_train": QuadSwarmConfig.sb_train(num_envs=4, num_agents=4),
            "n128": QuadSwarmConfig(num_envs=2, num_agents=128, neighbor_visible_num=6)}


@pytest.mark.parametrize("name", ["c3", "c4", "sb_train", "n128"])
def test_query_accepts_the_default(name):
    L = N.lib()
    rc = N.QsRenderConfig()
    assert L.qs_render_config_default(rc) == 0
    assert (rc.width, rc.height, rc.view, rc.follow, rc.drone_scale) == (256, 256, 0, 0, 1.0)
    nb = ctypes.c_size_t()
    assert L.qs_render_query(_configs()[name].to_qs_config(), rc, ctypes.byref(nb)) == 0, L.qs_last_error()
    assert nb.value == 256 * 256 * 3
    rc2 = RenderConfig(width=68, height=50, view="front", follow=True, drone_scale=4.0).to_qs()
    assert L.qs_render_query(_configs()[name].to_qs_config(), rc2, ctypes.byref(nb)) == 0
    assert nb.value == 68 * 50 * 3 and (rc2.view, rc2.follow) == (2, 1)


@pytest.mark.parametrize("field,value,msg", [("width", 66, b"multiple of 4"), ("width", 4096, b"[16, 2048]"),
                                             ("view", 7, b"view"), ("drone_scale", 0.0, b"drone_scale")])
def test_query_refusals(field, value, msg):
    L = N.lib()
    rc = N.QsRenderConfig()
    L.qs_render_config_default(rc)
    setattr(rc, field, value)
    nb = ctypes.c_size_t(7)
    assert L.qs_render_query(_configs()["c3"].to_qs_config(), rc, ctypes.byref(nb)) == -1
    assert msg in L.qs_last_error() and nb.value == 7
    others = {b"multiple of 4", b"[16, 2048]", b"view", b"drone_scale"} - {msg}
    assert not any(o in L.qs_last_error() for o in others)          # its own message


def test_query_more_refusals():
    L = N.lib()
    nb = ctypes.c_size_t()
    c3 = _configs()["c3"].to_qs_config()
    for field, value in (("height", 8), ("height", 2052), ("width", 12), ("view", -1), ("drone_scale", float("nan")),
                         ("drone_scale", float("inf")), ("drone_scale", 65.0)):
        rc = N.QsRenderConfig()
        L.qs_render_config_default(rc)
        setattr(rc, field, value)
        assert L.qs_render_query(c3, rc, ctypes.byref(nb)) == -1, (field, value)
    with pytest.raises(ValueError):
        RenderConfig(view="isometric").to_qs()


def test_palette_matches_the_header():
    src = open(os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd", "csrc", "qs_render.h")).read()
    body = re.search(r"QS_RENDER_PALETTE\[QS_PAL_N\]\[3\]\s*=\s*\{(.*?)\n\};", src, flags=re.S).group(1)
    rows = [tuple(int(v) for v in m) for m in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", body)]
    assert len(rows) == 37 == len(PALETTE) and PALETTE.dtype == np.uint8
    assert np.array_equal(np.array(rows), PALETTE)
    assert np.array_equal(PALETTE[16:32], PALETTE[:16] // 2)        # the half-intensity variants
    assert len({tuple(r) for r in PALETTE.tolist()}) == 37          # every entry tells something apart
    enums = dict(re.findall(r"(QS_PAL_\w+) = (\d+)", src))
    from quadswarm_amd import render as R
    assert [int(enums["QS_PAL_" + k]) for k in ("HALF", "OUTSIDE", "INSIDE", "OBSTACLE", "TARGET", "BORDER", "N")] == \
        [R.PAL_HALF, R.PAL_OUTSIDE, R.PAL_INSIDE, R.PAL_OBSTACLE, R.PAL_TARGET, R.PAL_BORDER, 37]


def test_tile_images_layouts():
    f = [np.full((2, 3, 3), k + 1, np.uint8) for k in range(4)]
    z = np.zeros((2, 3, 3), np.uint8)
    assert np.array_equal(tile_images(f[:1]), f[0])
    want3 = np.concatenate([np.concatenate([f[0], f[1]], axis=1), np.concatenate([f[2], z], axis=1)], axis=0)
    assert np.array_equal(tile_images(np.stack(f[:3])), want3) and want3.shape == (4, 6, 3)
    want4 = np.concatenate([np.concatenate([f[0], f[1]], axis=1), np.concatenate([f[2], f[3]], axis=1)], axis=0)
    assert np.array_equal(tile_images(f), want4)
    assert np.array_equal(tile_images(f, cols=4), np.concatenate(f, axis=1))
    assert tile_images(f).dtype == np.uint8


def test_write_png_decodes(tmp_path):
    frame = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    p = tmp_path / "f.png"
    write_png(str(p), frame)
    raw = p.read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    o, chunks = 8, []
    while o < len(raw):
        n, tag = struct.unpack(">I4s", raw[o:o + 8])
        data = raw[o + 8:o + 8 + n]
        assert struct.unpack(">I", raw[o + 8 + n:o + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        o += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (7, 5, 8, 2, 0, 0, 0)
    lines = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(5, 1 + 7 * 3)
    assert not lines[:, 0].any() and np.array_equal(lines[:, 1:].reshape(5, 7, 3), frame)
    with pytest.raises(ValueError):
        write_png(str(p), frame.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_should():
    by = {name: (s, w, h, kw) for name, s, w, h, kw in scenes()}
    s = by["b8_follow_side"][0]
    assert s["on_floor"].sum() == 1 and np.linalg.norm(s["pos"][3] - s["pos"][2]) < 2 * ARM     # overlapping
    assert np.abs(s["rot"][:, 2, 2]).max() < 0.999                                             # tilted
    assert np.abs(s["rot"][:, 0, 1]).max() > 0.3                                               # yawed
    for r in s["rot"]:
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-12)
    # the far drone sets the follow window: the rest sits well inside it
    c = s["pos"][:, [0, 2]].mean(0)
    d = np.abs(s["pos"][:, [0, 2]] - c).max(1)
    assert d.argmax() == 7 and np.sort(d)[-2] < 0.75 * d[7]
    assert by["n128_follow"][0]["pos"].shape[0] * 10 > 1024                                    # the chunked cull


def test_band_is_the_measured_displacement():
    disp, name = measured_displacement()
    print(f"measured displacement {disp:.3e} px (scene {name}) -> band {band():.3e} px")
    assert 0 < disp < 1e-3
    assert 0.5 * DOCUMENTED_DISPLACEMENT <= disp <= 2.0 * DOCUMENTED_DISPLACEMENT    # the docstring's figure is current
    assert band() == 4.0 * disp


@pytest.mark.parametrize("i", range(8))
def test_cap_and_fp32_agrees_with_fp64_outside_the_band(i):
    name = scenes()[i][0]
    f64, e64, _ = _restated(i, np.float64)
    f32, e32, _ = _restated(i, np.float32)
    banded = e64 <= band()
    print(f"{name}: {int(banded.sum())} of {banded.size} pixels in the band")
    assert banded.mean() <= CAP, name
    assert np.array_equal(f64[~banded], f32[~banded]), name
    assert f64.dtype == np.uint8 and f64.shape == (scenes()[i][3], scenes()[i][2], 3)


def test_restated_picture_has_every_layer():
    from quadswarm_amd import render as R
    by = {scenes()[i][0]: _restated(i, np.float64)[0] for i in range(8)}

    def has(frame, k):
        return bool((frame.reshape(-1, 3) == PALETTE[k]).all(1).any())
    f = by["c4_topdown"]
    assert all(has(f, k) for k in (R.PAL_OUTSIDE, R.PAL_INSIDE, R.PAL_OBSTACLE, R.PAL_BORDER, 0, 7))
    assert tuple(f[0, 0]) == tuple(PALETTE[R.PAL_OUTSIDE]) and has(f, 1 + R.PAL_HALF) and not has(f, 1)   # on the floor
    assert has(by["a4_target"], R.PAL_TARGET) and not has(by["b8_reset"], R.PAL_TARGET)
    assert has(by["c4_side"], R.PAL_OBSTACLE)
    # both lines beside a room edge on whole pixel coordinates are border (64 x 48, 10 m room: s = 4, edges at 4 / 44)
    f = by["b8_reset"]
    for r in (3, 4, 43, 44):
        assert tuple(f[r, 30]) == tuple(PALETTE[R.PAL_BORDER])
    assert tuple(f[2, 30]) == tuple(PALETTE[R.PAL_OUTSIDE]) and tuple(f[5, 30]) != tuple(PALETTE[R.PAL_BORDER])
