"""Seeded images for the tests of the built-in texture detector (tests/feature_reference.py): blocks with sharp
corners, a checker, a periodic pattern whose corners tie in score, and a smooth texture for descriptor tests."""
import numpy as np


def blocks(height, width, seed, n=60, low=4, high=14):
    """rectangles of random grey levels over a mid-grey ground, as BGR (the three channels differ)"""
    rng = np.random.default_rng(seed)
    image = np.full((height, width, 3), 110, np.uint8)
    for _ in range(n):
        h, w = rng.integers(low, high, 2)
        y, x = rng.integers(0, height - low), rng.integers(0, width - low)
        image[y:y + h, x:x + w] = rng.integers(0, 256, 3, dtype=np.uint8)
    return image


def checker(height, width, cell, origin=(0, 0), dark=40, bright=210):
    """grey checker (uint8): cell corners at origin + k * cell"""
    ys, xs = np.mgrid[0:height, 0:width]
    on = (((ys - origin[1]) // cell) + ((xs - origin[0]) // cell)) % 2 == 0
    return np.where(on, bright, dark).astype(np.uint8)


def squares(height, width, period, size, origin=(0, 0), ground=60, value=200):
    """bright squares of `size` pixels every `period` pixels on a dark ground (uint8): every square has four corners
    of equal score"""
    image = np.full((height, width), ground, np.uint8)
    for y in range(origin[1], height - size + 1, period):
        for x in range(origin[0], width - size + 1, period):
            image[y:y + size, x:x + size] = value
    return image


def as_bgr(grey):
    """a BGR image whose grey value (feature_reference.grey) is the given one: three equal channels"""
    return np.repeat(np.asarray(grey, np.uint8)[..., None], 3, axis=2)


def texture(size, seed, cells=10):
    """a smooth random texture (uint8, size x size) with a brightness ramp, so that the intensity centroid is off the
    centre by a clear margin"""
    rng = np.random.default_rng(seed)
    coarse = rng.uniform(0.0, 255.0, (cells + 3, cells + 3))
    at = np.linspace(1.0, cells + 1.0, size)
    i0 = np.floor(at).astype(int)
    a = at - i0
    rows = coarse[i0] * (1 - a)[:, None] + coarse[i0 + 1] * a[:, None]
    fine = rows[:, i0] * (1 - a)[None, :] + rows[:, i0 + 1] * a[None, :]
    ramp = np.linspace(-60.0, 60.0, size)[None, :]
    return np.clip(0.6 * fine + 50.0 + ramp, 0, 255).astype(np.uint8)


def turned(image, degrees):
    """the image turned about its centre pixel by the angle (counter-clockwise on the screen: x right, y down, a point
    at angle a moves to a - degrees), bilinear; what falls outside is mid-grey"""
    img = np.asarray(image, np.float64)
    h, w = img.shape
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    t = np.deg2rad(degrees)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sx = cx + (xs - cx) * np.cos(t) - (ys - cy) * np.sin(t)
    sy = cy + (xs - cx) * np.sin(t) + (ys - cy) * np.cos(t)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    ax, ay = sx - x0, sy - y0
    inside = (x0 >= 0) & (y0 >= 0) & (x0 < w - 1) & (y0 < h - 1)
    x0c, y0c = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    v = (img[y0c, x0c] * (1 - ax) * (1 - ay) + img[y0c, x0c + 1] * ax * (1 - ay) +
         img[y0c + 1, x0c] * (1 - ax) * ay + img[y0c + 1, x0c + 1] * ax * ay)
    return np.where(inside, np.rint(v), 128).astype(np.uint8)
