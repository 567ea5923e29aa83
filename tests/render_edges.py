"""Scenes for the focused renderers' kernels at mesh, image and geometry edges (csrc/m3t_render.hip): procedural meshes,
a case table, one function that builds a case behind either API, and the host-side tools the tests share -- the render
plan of csrc/m3t_render_plan.h as tests/cpp/render_plan_check.cpp prints it, the counters of tests/cpp/raster_stats.cpp,
and FocusedRenderer::CalculateProjectionMatrix restated in float32 operation for operation.

Units: a Frame turns focused-image pixels into metres for a body on the optical axis, so that a mesh can be written down
in pixels of the image it will be drawn into (u, v: integer = pixel centre)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import util
from util import host

F = np.float32
INTR = dict(fu=600.0, fv=600.0, ppu=320.0, ppv=240.0, width=640, height=480)
Z = 0.6          # depth of the bodies' origin
R = 0.1          # radius of the referenced body (octahedron, or a plate's corners)
COUNTERS = ("behind", "out_of_range", "zero_area", "culled", "no_centre", "survivors", "big", "big_per_trip", "covered",
            "depth_rejected", "ties", "w8", "w9", "box192", "box193", "wave_max", "empty_waves", "rule_rejected")
_MAXED = ("big_per_trip", "wave_max")  # per body: the kernels walk one body's list after the other

# ---- host tools ------------------------------------------------------------------------------------------------------
_tmp = None


def _tmpdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="m3t_render_edges_")
        atexit.register(shutil.rmtree, _tmp, True)
    return _tmp


def plan_exe():
    path = os.path.join(_tmpdir(), "render_plan_check")
    if not os.path.exists(path):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", path,
                        os.path.join(util.ROOT, "tests", "cpp", "render_plan_check.cpp")], check=True)
    return path


def plan(n_pairs, largest, image=None, env=None):
    """the project's own launch choice (m3t_render_plan.h) for such a launch under the case's overrides"""
    env = env or {}
    cmd = [plan_exe(), "--plan", str(n_pairs), str(largest)] + ([str(image)] if image is not None else [])
    if "M3T_HIP_RASTER_BANDS" in env:
        cmd += ["--bands", env["M3T_HIP_RASTER_BANDS"]]
    if "M3T_HIP_RASTER_SLICES" in env:
        cmd += ["--slices", env["M3T_HIP_RASTER_SLICES"]]
    if "M3T_HIP_NO_LDS_RASTER" in env:
        cmd += ["--no-lds"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=60, check=True).stdout
    d = dict(line.split() for line in out.splitlines())
    return {k: (v if k == "form" else int(v)) for k, v in d.items()}


_stats = None


def stats_lib():
    global _stats
    if _stats is None:
        so = os.path.join(_tmpdir(), "libraster_stats.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                        os.path.join(util.ROOT, "tests", "cpp", "raster_stats.cpp")], check=True)
        _stats = C.CDLL(so)
    return _stats


# ---- the crop and the transform, float32, operation for operation like focused_projection ----------------------------
def mul44(a, b):
    """the kernels' mul44: ((a0 b0 + a1 b1) + a2 b2) + a3 b3 per element, float32"""
    out = np.zeros((4, 4), F)
    for c in range(4):
        for r in range(4):
            out[r, c] = ((a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]) + a[r, 3] * b[3, c]
    return out


def maximum_body_diameter(vertices, geometry2body):
    """Body::CalculateMaximumBodyDiameter body.cpp:244-250: over the vertices in the body frame"""
    m = np.asarray(geometry2body, F).reshape(4, 4)
    v = np.asarray(vertices, F)
    q = [m[k, 3] + ((m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2]) for k in range(3)]
    return F(2.0) * np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]), dtype=F).max()


def focused_projection(intr, world2camera, referenced, S, z_min, z_max):
    """FocusedRenderer::CalculateProjectionMatrix renderer.cpp:348-405.  referenced: [(body2world, diameter)].
    Returns dict(corner_u, corner_v, scale, n_visible, visible, d, P)"""
    w2c = np.asarray(world2camera, F)
    fu, fv, ppu, ppv = F(intr["fu"]), F(intr["fv"]), F(intr["ppu"]), F(intr["ppv"])
    z_min, z_max = F(z_min), F(z_max)
    u_min, u_max, v_min, v_max = F(3.402823466e+38), F(1.175494351e-38), F(3.402823466e+38), F(1.175494351e-38)
    visible = []
    with np.errstate(all="ignore"):
        for b2w, diameter in referenced:
            t = np.asarray(b2w, F)[:3, 3]
            rr = F(0.5) * F(diameter)
            x = ((w2c[0, 0] * t[0] + w2c[0, 1] * t[1]) + w2c[0, 2] * t[2]) + w2c[0, 3]
            y = ((w2c[1, 0] * t[0] + w2c[1, 1] * t[1]) + w2c[1, 2] * t[2]) + w2c[1, 3]
            z = ((w2c[2, 0] * t[0] + w2c[2, 1] * t[1]) + w2c[2, 2] * t[2]) + w2c[2, 3]
            if z < rr * F(1.5) or z - rr < z_min or z + rr > z_max:
                visible.append(0)
                continue
            x2, y2, z2, r2 = x * x, y * y, z * z, rr * rr
            rz = rr * z
            z2_r2 = z2 - r2
            z3_zr2 = z2_r2 * z
            r_u = fu * (np.abs(x) * r2 + rz * np.sqrt(z2_r2 + x2, dtype=F)) / z3_zr2
            r_v = fv * (np.abs(y) * r2 + rz * np.sqrt(z2_r2 + y2, dtype=F)) / z3_zr2
            center_u = x * fu / z + ppu
            center_v = y * fv / z + ppv
            u_lo, u_hi, v_lo, v_hi = center_u - r_u, center_u + r_u, center_v - r_v, center_v + r_v
            if u_lo > F(intr["width"]) or u_hi < F(0) or v_lo > F(intr["height"]) or v_hi < F(0):
                visible.append(0)
                continue
            u_min, u_max = np.minimum(u_min, u_lo), np.maximum(u_max, u_hi)
            v_min, v_max = np.minimum(v_min, v_lo), np.maximum(v_max, v_hi)
            visible.append(1)
        out = dict(corner_u=F(0), corner_v=F(0), scale=F(1), n_visible=sum(visible), visible=visible, d=None,
                   P=np.zeros((4, 4), F))
        if out["n_visible"] == 0:
            return out
        d = np.maximum(u_max - u_min, v_max - v_min) * F(1.05)
        corner_u = F(0.5) * (u_min + u_max - d)
        corner_v = F(0.5) * (v_min + v_max - d)
        scale = F(S) / d
        P = out["P"]
        ppu_scaled = (ppu - corner_u) * scale
        ppv_scaled = (ppv - corner_v) * scale
        P[0, 0] = F(2.0) * fu / d
        P[0, 2] = F(2.0) * (ppu_scaled + F(0.5)) / F(S) - F(1.0)
        P[1, 1] = F(2.0) * fv / d
        P[1, 2] = F(2.0) * (ppv_scaled + F(0.5)) / F(S) - F(1.0)
        P[2, 2] = (z_max + z_min) / (z_max - z_min)
        P[2, 3] = F(-2.0) * z_max * z_min / (z_max - z_min)
        P[3, 2] = F(1.0)
        out.update(corner_u=corner_u, corner_v=corner_v, scale=scale, d=d)
    return out


def body_transform(P, world2camera, body2world, geometry2body):
    return mul44(P, mul44(np.asarray(world2camera, F), mul44(np.asarray(body2world, F), np.asarray(geometry2body, F))))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def drawn_triangles(body):
    """the index list as both APIs keep it: a clockwise mesh has every triangle's order reversed"""
    t = np.ascontiguousarray(body["t"], np.int32)
    return t if body["ccw"] else np.ascontiguousarray(t[:, ::-1])


def host_rendering(case, bodies, S, silhouette, id_type, world2camera=None, intr=INTR):
    """(depth, silhouette ids, projection) of the case's geometry with the device's own arithmetic on the host
    (raster_body of tests/cpp/raster_stats.cpp); bodies in draw order"""
    lib = stats_lib()
    w2c = np.eye(4, dtype=F) if world2camera is None else world2camera
    ref = [(b["pose"], maximum_body_diameter(b["v"], b["g2b"])) for b in bodies if b["ref"]]
    pr = focused_projection(intr, w2c, ref, S, case["z_min"], case["z_max"])
    packed = np.full(S * S, 0xFFFFFFFF, np.uint32)
    if pr["n_visible"]:
        for order, b in enumerate(bodies):
            trans = body_transform(pr["P"], w2c, b["pose"], b["g2b"])
            low = (order << 8) | ((b["region_id"] if id_type == 1 else b["body_id"]) if silhouette else 0)
            v, t = np.ascontiguousarray(b["v"], F), drawn_triangles(b)
            lib.raster_body(_fp(np.ascontiguousarray(trans.T)), _fp(v), _ip(t), len(t), int(b["culling"]), S, C.c_uint(low),
                            packed.ctypes.data_as(C.POINTER(C.c_uint)))
    depth = np.where(packed == 0xFFFFFFFF, 65535, packed >> 16).astype(np.uint16).reshape(S, S)
    sil = np.where(packed == 0xFFFFFFFF, 0, packed & 0xFF).astype(np.uint8).reshape(S, S)
    return depth, sil, pr


def case_stats(case, bodies, S, n_slices, world2camera=None, intr=INTR):
    """the counters of raster_edge_stats over the case's bodies (summed; the per-trip and per-wave maxima: the largest)"""
    lib = stats_lib()
    w2c = np.eye(4, dtype=F) if world2camera is None else world2camera
    ref = [(b["pose"], maximum_body_diameter(b["v"], b["g2b"])) for b in bodies if b["ref"]]
    pr = focused_projection(intr, w2c, ref, S, case["z_min"], case["z_max"])
    total = dict.fromkeys(COUNTERS, 0)
    per_body = []
    if pr["n_visible"]:
        for b in bodies:
            trans = body_transform(pr["P"], w2c, b["pose"], b["g2b"])
            out = np.zeros(24, np.int64)
            v, t = np.ascontiguousarray(b["v"], F), drawn_triangles(b)
            lib.raster_edge_stats(_fp(np.ascontiguousarray(trans.T)), _fp(v), _ip(t), len(t), int(b["culling"]), S,
                                  int(n_slices), out.ctypes.data_as(C.POINTER(C.c_longlong)))
            one = dict(zip(COUNTERS, (int(x) for x in out)))
            per_body.append(one)
            for k in COUNTERS:
                total[k] = max(total[k], one[k]) if k in _MAXED else total[k] + one[k]
    total["n_visible"] = pr["n_visible"]
    total["per_body"] = per_body
    return total


# ---- meshes ----------------------------------------------------------------------------------------------------------
class Frame:
    """focused-image pixels <-> metres in the plane z = 0 of a body at (0, 0, plane) when the referenced body stands at
    (0, 0, z) with radius r, for the
    camera INTR: u = x * K + S / 2 (integer u: a pixel centre).  From the crop's formulas in float64: good to a small
    fraction of a pixel, which is all a builder needs -- the tests count what the exact arithmetic makes of the mesh."""

    def __init__(self, S, z=Z, r=R, plane=None):
        d = 2.1 * INTR["fu"] * r / np.sqrt(z * z - r * r)
        self.S, self.K = S, S / d * INTR["fu"] / (z if plane is None else plane)  # plane: depth of the mesh's body

    def xy(self, u, v):
        return (u - 0.5 * self.S) / self.K, (v - 0.5 * self.S) / self.K


def plate(n, m, half_w, half_h, back=False, z=0.0):
    """a flat grid of n x m cells, two triangles per cell, facing the camera (back: facing away)"""
    xs, ys = np.linspace(-half_w, half_w, n + 1), np.linspace(-half_h, half_h, m + 1)
    gx, gy = np.meshgrid(xs, ys)
    v = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1).astype(F)
    i, j = np.meshgrid(np.arange(n), np.arange(m))
    a = (j * (n + 1) + i).ravel()
    b, c, d = a + 1, a + n + 1, a + n + 2
    t = np.stack([np.stack([a, d, b], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)  # negative area in the image: kept
    if back:
        t = t[:, ::-1]
    return v, np.ascontiguousarray(t, np.int32)


def with_triangles(mesh, n):
    """exactly n triangles: the first n of the mesh, or the mesh and its first triangles once more"""
    v, t = mesh
    while len(t) < n:
        t = np.concatenate([t, t[:n - len(t)]])
    return v, np.ascontiguousarray(t[:n])


def reversed_runs(mesh, run):
    """every second run of `run` consecutive triangles wound the other way"""
    v, t = mesh
    t = t.copy()
    odd = (np.arange(len(t)) // run) % 2 == 1
    t[odd] = t[odd][:, ::-1]
    return v, t


def octahedron(r=R):
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], F)
    t = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, t


def box(hx, hy, hz):
    v = np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], F)
    t = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2],
                  [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)
    return v, t


def stack(frame, k, corners, dz=1.0e-6):
    """k congruent triangles (corners: three (u, v) in pixels of the frame), each dz nearer than the one before"""
    pts = [frame.xy(u, v) for u, v in corners]
    v = np.array([[x, y, -i * dz] for i in range(k) for x, y in pts], F)
    t = np.arange(3 * k, dtype=np.int32).reshape(k, 3)
    if _image_area(corners) > 0:
        t = np.ascontiguousarray(t[:, ::-1])
    return v, t


def _image_area(c):
    return (c[1][0] - c[0][0]) * (c[2][1] - c[0][1]) - (c[1][1] - c[0][1]) * (c[2][0] - c[0][0])


def triangles_px(frame, tris, z=0.0):
    """triangles given by their corners in pixels, wound to face the camera"""
    v, t = [], []
    for tri in tris:
        order = tri if _image_area(tri) < 0 else tri[::-1]
        t.append([len(v), len(v) + 1, len(v) + 2])
        v += [list(frame.xy(u, w)) + [z] for u, w in order]
    return np.array(v, F), np.array(t, np.int32)


def slivers(frame, n=256):
    """one-row slivers 190 .. 196 pixels wide: boxes of exactly 192 and 193 pixels are among them"""
    tris = []
    for i in range(n):
        u0, v0, w = 2.0 + 0.013 * i, 20.0 + 0.55 * i, 189.5 + 0.4 * (i % 16)
        tris.append([(u0, v0 - 0.45), (u0 + w, v0), (u0, v0 + 0.45)])
    return triangles_px(frame, tris)


def rows_then_cells(frame, n_big, n_total):
    """n_big one-row slivers 195 pixels wide, each alone in its rows (a box over 192 pixels with pixels nobody else
    covers), then cells of a plate behind them up to n_total triangles, every box of those far below 192 pixels"""
    bv, bt = triangles_px(frame, [[(2.0, 10.0 + 2.2 * i - 0.9), (197.0, 10.0 + 2.2 * i), (2.0, 10.0 + 2.2 * i + 0.9)]
                                  for i in range(n_big)])
    half = 90.0 / frame.K
    pv, pt = with_triangles(plate(50, 26, half, half, z=0.02), n_total - n_big)
    return np.concatenate([bv, pv]), np.ascontiguousarray(np.concatenate([bt, pt + len(bv)]), np.int32)


def fan(frame, n=12, radius=60.0):
    """a fan around the image centre with degenerate members: a repeated index, three collinear vertices, and a
    triangle so small that its vertices snap to one point"""
    c = 0.5 * frame.S
    rim = [(c + radius * np.cos(2 * np.pi * k / n), c + radius * np.sin(2 * np.pi * k / n)) for k in range(n)]
    v = [list(frame.xy(c, c)) + [0.0]] + [list(frame.xy(u, w)) + [0.0] for u, w in rim]
    t = [[0, 1 + (k + 1) % n, 1 + k] for k in range(n)]
    t.insert(3, [0, 4, 4])                                                    # a repeated index
    first = len(v)
    v += [list(frame.xy(c - 40 + 30 * k, c + 10.0)) + [0.0] for k in range(3)]   # collinear: one image row
    t.insert(7, [first, first + 1, first + 2])
    first = len(v)
    v += [list(frame.xy(c + 20.3 + 1e-4 * k, c - 20.3 + 1e-4 * (k % 2))) + [0.0] for k in range(3)]  # < 1/256 pixel
    t.append([first, first + 1, first + 2])
    return np.array(v, F), np.array(t, np.int32)


def rot_x(deg):
    a = np.deg2rad(deg)
    m = np.eye(4, dtype=F)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return m


def rot_z(deg):
    a = np.deg2rad(deg)
    m = np.eye(4, dtype=F)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return m


def at(x=0.0, y=0.0, z=Z, rotation=None):
    m = np.eye(4, dtype=F) if rotation is None else rotation.astype(F).copy()
    m[:3, 3] = (x, y, z)
    return m


def body(mesh, pose=None, g2b=None, body_id=100, region_id=None, culling=True, ccw=True, ref=True):
    return dict(v=mesh[0], t=mesh[1], pose=at() if pose is None else pose, g2b=np.eye(4, dtype=F) if g2b is None else g2b,
                body_id=body_id, region_id=body_id if region_id is None else region_id, culling=culling, ccw=ccw, ref=ref)


H = R / np.sqrt(2.0)  # half side of a square plate whose corners lie at the radius R


def square(n, m=None, **kw):
    return plate(n, n if m is None else m, H, H, **kw)


# ---- the case table --------------------------------------------------------------------------------------------------
def case(name, bodies, S=200, env=None, path="start", live=None, drawn=True, z_min=0.02, z_max=10.0, id_type=0,
         moved=None, **extra):
    """path "start": one silhouette renderer through StartRendering; "tracker": renderers of a region modality, drawn by
    StartModalities (pairs and twins).  live(st, pl): the property the case exists for, from the counters (st) and the
    plan (pl); returns what to print.  moved: a second rendering after body 0 took this pose."""
    return dict(name=name, bodies=bodies, S=S, env=dict(env or {}), path=path, live=live, drawn=drawn, z_min=z_min,
                z_max=z_max, id_type=id_type, moved=moved, **extra)


NO_LDS = {"M3T_HIP_NO_LDS_RASTER": "1"}


def _slices(n):
    return {"M3T_HIP_RASTER_SLICES": str(n)}


def _bands(n):
    return {"M3T_HIP_RASTER_BANDS": str(n)}


def _need(cond, text):
    assert cond, text
    return text


def _trips(n, slices, want):
    per = -(-n // slices)

    def live(st, pl):
        trips = -(-per // 512)
        return _need(pl["form"] == "lds" and pl["slices"] == slices and trips == want and st["survivors"] > 0,
                     "%d triangles in %d slices: %d trips of 512, %d survivors" % (n, slices, trips, st["survivors"]))
    return live


def _survivors(n, at_least=False):
    def live(st, pl):
        ok = st["survivors"] >= n if at_least else st["survivors"] == n
        return _need(pl["form"] == "lds" and ok, "%d survivors: %d resolve trips of 2048" %
                     (st["survivors"], -(-st["survivors"] // 2048)))
    return live


def _plan_is(**want):
    def live(st, pl):
        return _need(all(pl[k] == v for k, v in want.items()) and (st["covered"] > 0),
                     " ".join("%s %s" % (k, pl[k]) for k in sorted(want)) + ", %d covered pixels" % st["covered"])
    return live


def _queue(per_trip):
    def live(st, pl):
        return _need(pl["form"] == "three" and st["big_per_trip"] == per_trip,
                     "%d boxes over 192 pixels in one trip of a slice (queue of 64)" % st["big_per_trip"])
    return live


def _three_trips(n, want):
    def live(st, pl):
        trips = -(-(-(-n // 32)) // 512)
        return _need(pl["form"] == "three" and pl["slices"] == 32 and trips == want and st["survivors"] > 0,
                     "%d triangles in 32 slices: %d trips" % (n, trips))
    return live


def _counter(name, form=None, at_least=1, drawn=True):
    def live(st, pl):
        return _need(st[name] >= at_least and (st["covered"] > 0) == drawn and (form is None or pl["form"] == form),
                     "%s %d, covered %d, form %s" % (name, st[name], st["covered"], pl["form"]))
    return live


def _anchor(**kw):
    return body(octahedron(), body_id=kw.pop("body_id", 7), **kw)


def _cases():
    out = []
    # ---- a. set-up trips (LDS form) ----
    for n, trips in ((1, 1), (511, 1), (512, 1), (513, 2), (1024, 2), (1025, 3), (1537, 4)):
        out.append(case("setup_slices1_%d" % n, [body(with_triangles(square(28), n))], env=_slices(1),
                        live=_trips(n, 1, trips)))
    out.append(case("setup_slices3_1537", [body(with_triangles(square(28), 1537))], env=_slices(3), live=_trips(1537, 3, 2)))
    out.append(case("setup_default_2_triangles", [body(with_triangles(square(1), 2))], live=_trips(2, 128, 1)))

    def waves(st, pl):
        return _need(st["culled"] == 512 and st["empty_waves"] == 8 and st["wave_max"] == 64 and pl["slices"] == 1,
                     "culled %d, %d waves without and 8 with 64 survivors" % (st["culled"], st["empty_waves"]))
    out.append(case("setup_waves_without_survivors", [body(reversed_runs(with_triangles(square(23), 1024), 64))],
                    env=_slices(1), live=waves))

    def two(st, pl):
        n = [b["survivors"] for b in st["per_body"]]
        return _need(n[0] == 513 and 0 < n[1] <= 3, "survivors per body %s" % n)
    out.append(case("setup_two_bodies_513_and_3",
                    [body(with_triangles(square(17), 513)),
                     body(with_triangles(plate(2, 1, 0.5 * H, 0.25 * H, z=-0.01), 3), body_id=33, ref=False)],
                    env=_slices(1), live=two))
    # ---- b. resolve trips ----
    out.append(case("resolve_0_survivors", [body(square(8, back=True))], drawn=False,
                    live=lambda st, pl: _need(st["survivors"] == 0 and st["culled"] == 128 and st["n_visible"] == 1,
                                              "0 survivors of a visible body, culled %d" % st["culled"])))
    out.append(case("resolve_1_survivor", [body(with_triangles(square(2), 1))], live=_survivors(1)))
    out.append(case("resolve_2047_survivors", [body(with_triangles(square(32), 2047))], live=_survivors(2047)))
    out.append(case("resolve_2048_survivors", [body(square(32))], live=_survivors(2048)))
    out.append(case("resolve_2049_survivors", [body(with_triangles(square(33, 32), 2049))], live=_survivors(2049)))
    out.append(case("resolve_4097_survivors", [body(with_triangles(square(46), 4097))], live=_survivors(4097)))
    f, front = Frame(200), Frame(200, plane=Z - 0.11)  # front: of a body that stands before the referenced octahedron

    def beside(st, pl):
        big = st["per_body"][1]
        return _need(st["survivors"] >= 2049 and big["survivors"] == 1 and big["covered"] > 8000,
                     "%d survivors, one of them covering %d pixels" % (st["survivors"], big["covered"]))
    out.append(case("resolve_one_large_beside_small",
                    [body(square(34)), body(triangles_px(f, [[(4, 3), (196, 5), (6, 197)]], z=0.004), body_id=9, ref=False)],
                    live=beside))

    def widths(st, pl):
        return _need(st["w8"] > 0 and st["w9"] > 0, "boxes 8 wide: %d, 9 wide: %d" % (st["w8"], st["w9"]))
    out.append(case("resolve_boxes_8_and_9_wide", [body(square(16))], live=widths))
    # ---- c. bands and stores ----
    for S, want in ((8, dict(vector_bands=8, one_row_bands=8)), (9, dict(scalar_bands=5, one_row_bands=1, empty_bands=3)),
                    (10, dict(vector_bands=5, empty_bands=3)), (13, dict(scalar_bands=7, one_row_bands=1, empty_bands=1)),
                    (64, dict(vector_bands=32)), (201, dict(scalar_bands=67, empty_bands=33)),
                    (1024, dict(vector_bands=256, bands=256))):
        out.append(case("bands_default_%d" % S, [body(square(8))], S=S, live=_plan_is(form="lds", **want)))
    out.append(case("bands_4_at_13", [body(square(8))], S=13, env=_bands(4),
                    live=_plan_is(form="lds", vector_bands=3, scalar_bands=1, one_row_bands=1, partial_bands=1)))
    out.append(case("bands_1_at_64", [body(square(8))], S=64, env=_bands(1), live=_plan_is(form="lds", bands=1, vector_bands=1)))
    out.append(case("bands_mixed_8_and_333", [body(square(8), culling=False)], path="tracker", S=333, twin_S=8, order="depth_first",
                    live=lambda st, pl: _need(pl["bands"] == 128 and pl["small"]["empty_bands"] == 120 and st["covered"] > 0,
                                              "128 bands: the renderer of 8 rows leaves 120 empty")))
    # ---- d. twins ----
    three = [body(square(8), body_id=150, region_id=20, culling=False),
             body(box(0.3 * H, 0.6 * H, 0.01), pose=None, body_id=50, region_id=21, ref=False),  # reaches the last row
             body(octahedron(0.03), body_id=7, region_id=22, ref=False)]
    for name, kw in (("twins_depth_first", dict(order="depth_first")), ("twins_silhouette_first", dict(order="silhouette_first")),
                     ("twins_region_ids", dict(order="depth_first", id_type=1)),
                     ("twins_region_ids_silhouette_first", dict(order="silhouette_first", id_type=1)),
                     ("twins_13_bands_4", dict(order="depth_first", id_type=1, S=13, env=_bands(4))),
                     ("twins_13_bands_4_silhouette_first", dict(order="silhouette_first", id_type=1, S=13, env=_bands(4)))):
        def twins(st, pl, kw=kw):
            return _need(pl["pairs"] == 1 and pl["twin"] and st["covered"] > 0 and
                         all(b["covered"] > 0 for b in st["per_body"]),
                         "one pair with a twin, bodies cover %s, stores: %d vector %d scalar bands" %
                         ([b["covered"] for b in st["per_body"]], pl["vector_bands"], pl["scalar_bands"]))
        offsets = [None, (0.02, 0.08, -0.05), (-0.03, 0.02, -0.08)]
        if kw["order"] == "silhouette_first":  # another scene: what the case before left in memory is not this one's image
            offsets = [None, (-0.02, 0.08, -0.05), (0.03, -0.02, -0.08)]
        out.append(case(name, three, path="tracker", live=twins, offsets=offsets, last_row=True, **kw))
    # ---- e. the three-launch form ----
    f64 = Frame(64)
    big = [(6, 5), (58, 9), (9, 57)]
    for name, k, per_trip in (("three_queue_overflow_2560", 2560, 80), ("three_queue_full_2048", 2048, 64),
                              ("three_queue_one_over_2080", 2080, 65)):
        out.append(case(name, [_anchor(), body(stack(f64, k, big), body_id=200, ref=False)], S=64, env=NO_LDS,
                        live=_queue(per_trip)))

    # the same with pixels of their own for every queued triangle: the first slice holds the large ones, 80 / 65 / 64 of them
    for name, k, n in (("three_queue_overflow_own_rows", 80, 2560), ("three_queue_one_over_own_rows", 65, 2080),
                       ("three_queue_full_own_rows", 64, 2048)):
        def own(st, pl, k=k):
            own = st["per_body"][1]
            return _need(pl["form"] == "three" and own["big_per_trip"] == k == own["big"],
                         "%d boxes over 192 pixels, all in the first slice's trip, each alone in its rows" % own["big"])
        out.append(case(name, [_anchor(), body(rows_then_cells(front, k, n), pose=at(z=Z - 0.11), body_id=200, ref=False)],
                        env=NO_LDS, live=own))

    def boxes(st, pl):
        return _need(pl["form"] == "three" and st["box192"] > 0 and st["box193"] > 0,
                     "boxes of exactly 192 pixels: %d, of 193: %d" % (st["box192"], st["box193"]))
    out.append(case("three_boxes_192_and_193", [_anchor(), body(slivers(front), pose=at(z=Z - 0.11), body_id=200, ref=False)],
                    env=NO_LDS, live=boxes))
    out.append(case("three_two_trips_18432", [body(square(96))], env=NO_LDS, live=_three_trips(18432, 2)))
    out.append(case("three_three_trips_33800", [body(square(130))], env=NO_LDS, live=_three_trips(33800, 3)))
    out.append(case("three_nothing_visible", [body(square(8), pose=at(z=0.12))], env=NO_LDS, drawn=False,
                    live=lambda st, pl: _need(st["n_visible"] == 0 and pl["form"] == "three", "n_visible 0")))
    out.append(case("three_image_8", [body(square(8))], S=8, env=NO_LDS, live=_counter("covered", "three")))
    out.append(case("three_image_1024", [body(square(8))], S=1024, env=NO_LDS, live=_counter("covered", "three")))
    out.append(case("three_second_rendering", [body(square(8)), _anchor(pose=at(0.02, 0.01, Z + 0.2), ref=False)], env=NO_LDS,
                    moved=at(0.05, -0.04, 0.9, rot_z(30.0)), live=_counter("covered", "three")))
    # ---- f. geometry, both forms ----
    for form, env in (("lds", {}), ("three", NO_LDS)):
        def g(name, bodies, live, **kw):
            out.append(case("geometry_%s_%s" % (name, form), bodies, env=env, live=live, **kw))
        tilted = plate(6, 6, 0.3, 0.3)
        g("occluder_across_camera_plane", [_anchor(), body(tilted, pose=at(z=0.0, rotation=rot_x(60.0)), body_id=9, ref=False,
                                                           culling=False)], _counter("behind", form))
        g("occluder_before_z_min", [_anchor(), body(plate(2, 2, 0.004, 0.004), pose=at(z=0.01), body_id=9, ref=False)],
          _counter("depth_rejected", form))
        g("occluder_across_z_min", [_anchor(), body(plate(4, 4, 0.01, 0.01), pose=at(z=0.02, rotation=rot_x(60.0)), body_id=9,
                                                    ref=False, culling=False)], _counter("depth_rejected", form))
        g("occluder_across_z_max", [_anchor(), body(tilted, pose=at(z=1.0, rotation=rot_x(60.0)), body_id=9, ref=False,
                                                    culling=False)], _counter("depth_rejected", form), z_max=1.0)
        near = (np.array([[0.1, 0.0, 1.0e-6], [0.0, 0.02, 0.5], [0.0, -0.02, 0.5], [0.05, 0.0, 0.5]], F),
                np.array([[0, 1, 2], [3, 2, 1]], np.int32))
        g("vertex_off_the_integer_range", [_anchor(), body(near, pose=at(z=0.0), body_id=9, ref=False, culling=False)],
          _counter("out_of_range", form))
        g("degenerate_fan", [_anchor(), body(fan(front), pose=at(z=Z - 0.11), body_id=9, ref=False)], _counter("zero_area", form, 3))
        cw = (square(8)[0], square(8)[1][:, ::-1])
        g("clockwise_culling_on", [body(cw, ccw=False)], _counter("survivors", form, 128))
        g("clockwise_culling_off", [body(cw, ccw=False, culling=False)], _counter("survivors", form, 128))
        g("counterclockwise_back_culling_off", [body(square(8, back=True), culling=False)], _counter("survivors", form, 128))
        shift = rot_z(25.0) @ rot_x(20.0)
        shift[:3, 3] = (0.01, -0.02, 0.015)
        g("geometry2body_rotated", [body(box(0.04, 0.03, 0.02), g2b=shift.astype(F))], _counter("culled", form))
        for order in ((11, 12), (12, 11)):
            def first_owns(st, pl, order=order):
                a, b = st["per_body"]
                return _need(a["covered"] == b["covered"] > 0, "both bodies cover the same %d pixels" % a["covered"])
            g("equal_depth_ids_%d_%d" % order, [body(square(4), body_id=order[0]), body(square(4), body_id=order[1])],
              first_owns, owner=order[0])
        g("ids_0_and_255", [body(plate(4, 4, H, 0.4 * H), pose=at(y=-0.03), body_id=255),
                            body(plate(4, 4, 0.5 * H, 0.3 * H), pose=at(y=0.04), body_id=0, ref=False)],
          lambda st, pl: _need(all(b["covered"] > 0 for b in st["per_body"]), "both drawn"), ids={255})
        eight = [_anchor(pose=at(z=Z + 0.12))] + [
            body(octahedron(0.02), pose=at(0.035 * (k % 4) - 0.05, 0.05 * (k // 4) - 0.025, Z - 0.01 * k), body_id=10 + k,
                 ref=False) for k in range(1, 8)]
        g("eight_bodies", eight, lambda st, pl: _need(len(st["per_body"]) == 8 and all(b["covered"] > 0 for b in st["per_body"]),
                                                       "8 bodies drawn"))
        hidden = {2: at(0.0, 0.0, 0.04), 4: at(0.0, 0.0, 0.048, rot_z(10.0)), 6: at(1.2, 0.0, 0.5)}  # 1.5 r | z_min | off-image
        many = [body(octahedron(0.03), pose=hidden.get(k, at(0.06 * (k % 4) - 0.09, 0.07 * (k // 4) - 0.03, Z + 0.01 * k)),
                     body_id=10 + k) for k in range(8)]
        g("eight_referenced_three_invisible", many, lambda st, pl: _need(st["n_visible"] == 5, "5 of 8 visible"), z_min=0.02)
        lone, lone_pose = bottom_edge_pose(front)
        g("bottom_edge_on_pixel_centres", [_anchor(), body(lone, pose=lone_pose, body_id=9, ref=False)],
          _counter("rule_rejected", form, 50))
        g("vertices_on_pixel_centres", [body(square(8), pose=tie_pose())], _counter("ties", form))
    return out


_tie = None


def tie_pose():
    """a pose of the 8 x 8 plate under which covered pixels have an edge function of exactly 0: the first of a few seeded
    candidates that has such ties (searched on the host; the CPU test asserts the count)"""
    global _tie
    if _tie is None:
        probe = dict(z_min=0.02, z_max=10.0)
        rng = np.random.default_rng(5)
        best = (0, at())
        for k in range(24):
            pose = at(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), Z + rng.uniform(-0.1, 0.1)) if k else at()
            st = case_stats(probe, [body(square(8), pose=pose)], 200, 128)
            if st["ties"] > best[0]:
                best = (st["ties"], pose)
        _tie = best[1]
    return _tie


_bottom = None


def bottom_edge_pose(frame):
    """a pose of one large triangle, in front of the referenced octahedron, whose horizontal bottom edge lies exactly on
    a row of pixel centres: those pixels belong to whatever lies below (searched on the host in steps of 1 / 512 pixel:
    the snapped coordinates have 256 values per pixel)"""
    global _bottom
    if _bottom is None:
        probe = dict(z_min=0.02, z_max=10.0)
        mesh = triangles_px(frame, [[(40.0, 40.0), (160.0, 150.0), (60.0, 150.0)]])
        for k in range(1024):
            pose = at(y=k / 512.0 / frame.K, z=Z - 0.11)
            st = case_stats(probe, [_anchor(), body(mesh, pose=pose, body_id=9, ref=False)], frame.S, 128)
            if st["per_body"][1]["rule_rejected"] >= 50:
                _bottom = (mesh, pose)
                break
    return _bottom


_table = None


def cases():
    global _table
    if _table is None:
        _table = _cases()
        names = [c["name"] for c in _table]
        assert len(set(names)) == len(names)
    return _table


def case_named(name):
    return next(c for c in cases() if c["name"] == name)


# ---- a case behind either API ----------------------------------------------------------------------------------------
class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _make_body(api, b, existing=None):
    h = existing if existing is not None else host.Body(api, b["pose"])
    h.set_geometry(b["v"], b["t"], b["g2b"], geometry_counterclockwise=b["ccw"], geometry_enable_culling=b["culling"],
                   body_id=b["body_id"], region_id=b["region_id"])
    return h


def tracker_bodies(c):
    """the bodies of a tracker-path case with their poses: body 0 stands where the fixture's body stands, the others are
    offset from it in the camera frame"""
    import golden_scene as gs
    base = np.asarray(gs.mtv.body2world(), F)
    out = []
    for k, b in enumerate(c["bodies"]):
        pose = base.copy()
        offset = (c.get("offsets") or [None] * len(c["bodies"]))[k]
        if offset is not None:
            pose[:3, 3] = pose[:3, 3] + np.asarray(offset, F)
        out.append(dict(b, pose=pose))
    return out


def render_case(api, c):
    """Builds the case behind `api` and renders it.  Returns a list of renderings, one per renderer and rendering:
    (name, (depth, silhouette or None, corner_u, corner_v, scale, n_visible))"""
    out = []
    with _Env(c["env"] if api.is_hip else {}):
        if c["path"] == "start":
            bodies = [_make_body(api, b) for b in c["bodies"]]
            camera = host.ColorCamera(api, **INTR)
            geometry = host.RendererGeometry(api)
            for h in bodies:
                geometry.AddBody(h)
            r = host.FocusedSilhouetteRenderer(api, geometry, camera, id_type=c["id_type"], image_size=c["S"],
                                               z_min=c["z_min"], z_max=c["z_max"])
            for h, b in zip(bodies, c["bodies"]):
                if b["ref"]:
                    r.AddReferencedBody(h)
            r.StartRendering()
            out.append(("silhouette", r.images()))
            if c["moved"] is not None:
                bodies[0].set_body2world_pose(c["moved"])
                r.StartRendering()
                out.append(("silhouette, moved", r.images()))
        else:
            import golden_scene as gs
            f = gs.TrackerFixture(api, measure_occlusions=False, region_params=dict(n_unoccluded_iterations=0),
                                  depth_params=dict(n_unoccluded_iterations=0))
            specs = tracker_bodies(c)
            bodies = [_make_body(api, specs[0], existing=f.body)] + [_make_body(api, b) for b in specs[1:]]
            geometry = host.RendererGeometry(api)
            for h in bodies:
                geometry.AddBody(h)

            def depth():
                return host.FocusedBasicDepthRenderer(api, geometry, f.color_camera, image_size=c["S"], z_min=c["z_min"],
                                                      z_max=c["z_max"])

            def silhouette():
                return host.FocusedSilhouetteRenderer(api, geometry, f.color_camera, id_type=c["id_type"],
                                                      image_size=c.get("twin_S", c["S"]), z_min=c["z_min"], z_max=c["z_max"])
            if c["order"] == "depth_first":
                d = depth()
                s = silhouette()
            else:
                s = silhouette()
                d = depth()
            for r in (d, s):
                r.AddReferencedBody(f.body)
            f.region.ModelOcclusions(d)
            f.region.UseRegionChecking(s)
            assert f.tracker.StartModalities(0)
            out.append(("depth", d.images()))
            out.append(("silhouette", s.images()))
    return out


# ---- g. the crop sweep -----------------------------------------------------------------------------------------------
SWEEP_S, SWEEP_Z_MAX = 8, 1.0
SWEEP_Z_MIN = (0.02, 0.1)  # of the sweep's two renderers: z - r = z_min lies behind z = 1.5 r only for the second


def sweep_projection(pose, which):
    ref = [(pose, maximum_body_diameter(octahedron()[0], np.eye(4, dtype=F)))]
    return focused_projection(INTR, np.eye(4, dtype=F), ref, SWEEP_S, SWEEP_Z_MIN[which], SWEEP_Z_MAX)


def _flip(lo, hi, make, which):
    """four consecutive float32 values in [lo, hi]: the visibility of make(value) changes between the second and the
    third (bisection over the bit patterns of positive floats)"""
    def visible(bits):
        return sweep_projection(make(np.array(bits, np.int32).view(F)[()]), which)["n_visible"] == 1
    a, b = int(np.array(lo, F).view(np.int32)), int(np.array(hi, F).view(np.int32))
    va = visible(a)
    assert va != visible(b)
    while b - a > 1:
        mid = (a + b) // 2
        if visible(mid) == va:
            a = mid
        else:
            b = mid
    return [np.array(k, np.int32).view(F)[()] for k in (a - 1, a, b, b + 1)]


def sweep_poses():
    """256 (pose, renderer) of the octahedron: four consecutive float32 values around each visibility threshold (z = 1.5 r,
    z - r = z_min, z + r = z_max, u_min_body = width, v_min_body = height; `groups` are their index ranges, the outcome
    changes inside each), then seeded poses across the frustum and partly outside it"""
    poses, groups = [], []

    def z_only(z):
        return at(0.0, 0.0, z)
    for lo, hi, make, which in ((0.1, 0.2, z_only, 0),                               # z = 1.5 r
                                (0.16, 0.4, z_only, 1),                              # z - r = z_min = 0.1
                                (0.5, 0.95, z_only, 0),                              # z + r = z_max
                                (0.3, 0.9, lambda x: at(x, 0.0, 0.8), 0),            # u_min_body = width
                                (0.2, 0.7, lambda y: at(0.0, y, 0.8), 0)):           # v_min_body = height
        groups.append((len(poses), len(poses) + 4))
        poses += [(make(v), which) for v in _flip(lo, hi, make, which)]
    rng = np.random.default_rng(11)
    while len(poses) < 256:
        a, b = rng.uniform(0, 360, 2)
        poses.append((at(rng.uniform(-0.9, 0.9), rng.uniform(-0.7, 0.7), rng.uniform(0.1, 1.3), rot_z(a) @ rot_x(b)),
                      len(poses) % 2))
    return poses, groups


def render_sweep(api, poses):
    """one context, two renderers of one geometry, the poses set in a loop"""
    b = host.Body(api, poses[0][0])
    b.set_geometry(*octahedron(), body_id=77)
    camera = host.ColorCamera(api, **INTR)
    geometry = host.RendererGeometry(api)
    geometry.AddBody(b)
    renderers = [host.FocusedSilhouetteRenderer(api, geometry, camera, image_size=SWEEP_S, z_min=z_min, z_max=SWEEP_Z_MAX)
                 for z_min in SWEEP_Z_MIN]
    for r in renderers:
        r.AddReferencedBody(b)
    out = []
    for pose, which in poses:
        b.set_body2world_pose(pose)
        renderers[which].StartRendering()
        out.append(renderers[which].images())
    return out


# ---- what the tests ask of a case -----------------------------------------------------------------------------------
def case_scene(c):
    """(bodies with the poses they are drawn at, intrinsics) of a case; the cameras' world2camera is the identity"""
    if c["path"] == "start":
        return c["bodies"], INTR
    import golden_scene as gs
    return tracker_bodies(c), gs.mtv.COLOR_INTRINSICS


def case_plan(c):
    """the launch the library chooses for the case, from its own rule"""
    if c["path"] == "start":
        pl = plan(1, c["S"], env=c["env"])
        pl.update(pairs=1, twin=False)
        return pl
    small = c.get("twin_S", c["S"])
    pairs = 1 if small == c["S"] else 2
    pl = plan(pairs, max(small, c["S"]), image=c["S"], env=c["env"])
    pl.update(pairs=pairs, twin=pairs == 1, small=plan(pairs, max(small, c["S"]), image=small, env=c["env"]))
    return pl
