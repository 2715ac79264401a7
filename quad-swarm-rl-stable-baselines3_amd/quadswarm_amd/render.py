"""Host side of the headless renderer (qs_render, csrc/qs_render.h): its configuration, the palette, and the two
helpers a video loop needs -- SB3's tile_images layout and a PNG writer on the standard library.

    frames = env.render(env_ids=[0, 1], cfg=RenderConfig(width=256, height=256, view="topdown", drone_scale=4.0))
    write_png("frame_000.png", tile_images(frames.cpu().numpy()))

The frames are drawn on the device from the state the step kernels keep there; DESIGN.md ("Rendering") has the
picture's contract.  numpy only: nothing here needs torch or an image library.
"""
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import _native as N

# csrc/qs_render.h QS_RENDER_PALETTE: 16 drone colours (drone i draws in PALETTE[i % 16]), their half-intensity
# variants (rear rotors, drones on the floor), then the fixed colours
PALETTE = np.array([
    (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200),
    (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
    (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255),
    (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
    (115, 12, 37), (30, 90, 37), (127, 112, 12), (0, 65, 100),
    (122, 65, 24), (72, 15, 90), (35, 120, 120), (120, 25, 115),
    (105, 122, 30), (125, 95, 106), (0, 64, 64), (110, 95, 127),
    (85, 55, 20), (127, 125, 100), (64, 0, 0), (85, 127, 97),
    (24, 24, 28), (52, 54, 60), (150, 150, 158), (255, 255, 255),
    (200, 200, 205),
], dtype=np.uint8)
PAL_HALF, PAL_OUTSIDE, PAL_INSIDE, PAL_OBSTACLE, PAL_TARGET, PAL_BORDER = 16, 32, 33, 34, 35, 36


@dataclass
class RenderConfig:
    width: int = 256              # 16..2048, a multiple of 4
    height: int = 256             # 16..2048
    view: str = "topdown"         # "topdown" (x, y), "side" (x, z), "front" (y, z)
    follow: bool = False          # False: the room fills the frame; True: a square window around the drones
    drone_scale: float = 1.0      # magnifies the drones (not the room, pillars or capture ring); a 10 m room wants ~4

    def to_qs(self):
        if self.view not in N.RENDER_VIEWS:
            raise ValueError(f"view must be one of {sorted(N.RENDER_VIEWS)}, got {self.view!r}")
        rc = N.QsRenderConfig()
        N.check(N.lib().qs_render_config_default(rc), "qs_render_config_default")
        rc.width, rc.height = int(self.width), int(self.height)
        rc.view, rc.follow, rc.drone_scale = N.RENDER_VIEWS[self.view], int(bool(self.follow)), float(self.drone_scale)
        return rc


def tile_images(frames, cols=None):
    """n frames [n, H, W, C] (an array or a sequence of [H, W, C]) as one [rows * H, cols * W, C] image, row-major,
    the unused cells black: stable_baselines3.common.vec_env.base_vec_env.tile_images' layout (rows =
    ceil(sqrt(n)), cols = ceil(n / rows)) unless `cols` is given."""
    a = np.asarray(frames)
    if a.ndim != 4 or a.shape[0] < 1:
        raise ValueError("tile_images wants [n, H, W, C] with n >= 1")
    n, h, w, c = a.shape
    if cols is None:
        rows = int(np.ceil(np.sqrt(n)))
        cols = int(np.ceil(n / rows))
    else:
        cols = int(cols)
        if cols < 1:
            raise ValueError("cols must be >= 1")
        rows = -(-n // cols)
    out = np.zeros((rows * cols, h, w, c), dtype=a.dtype)
    out[:n] = a
    return out.reshape(rows, cols, h, w, c).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, c)


def write_png(path, frame):
    """Write one uint8 [H, W, 3] (RGB) or [H, W] (grey) frame as a PNG: 8 bits per channel, no filter, zlib."""
    a = np.ascontiguousarray(frame)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("write_png wants a uint8 [H, W, 3] or [H, W] array")
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + a.size // h), dtype=np.uint8)    # each scanline: filter byte 0, then the pixels
    raw[:, 1:] = a.reshape(h, -1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)) +
           chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


__all__ = ["RenderConfig", "PALETTE", "tile_images", "write_png"]
