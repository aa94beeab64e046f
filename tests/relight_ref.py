"""Test-only restatement of the relight rules (include/rtmi_relight.h, csrc/rtmi_relight.hpp) in numpy f64 with explicit
loops, the light lists the CPU and GPU tests share, and the calls of rtml_relight_desc."""
import ctypes as C
import math

import numpy as np

import refit_ref as R
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import LIGHT_NODE_DTYPE

LIGHT = np.dtype([("item", "<i4"), ("prim", "<i4"), ("kind", "<i4"), ("material", "<i4"), ("area", "<f8"), ("weight", "<f8"),
                  ("select_p", "<f8"), ("cdf", "<f8")])
# the device's record of a light (csrc/rtmi_shade.hpp, NeeLight)
DEV_LIGHT = np.dtype([("geo", "<f4", 4), ("k", "<f4"), ("plane", "<i4"), ("item", "<i4"), ("prim", "<i4"), ("area", "<f4"),
                      ("p_sel", "<f4"), ("cdf", "<f4"), ("pad", "<i4")])
LEAF = 0x80000000
PLANE_SHIFT = 8  # RTMI_PRIMFLAG_PLANE_SHIFT of include/rtmi.h
COUNTS = (1, 2, 3, 65, 257)
f64 = np.float64


def light_list(host, n, seed=1):
    """A floor and n emitters in one list item: rects of all three planes and spheres in turn, SOLID emitters of unequal
    weights, and every fifth light a checker emitter (not SOLID: weight 1).  -> world"""
    rng = np.random.default_rng(seed)
    world = host.HittableList()
    world.push(host.Rect(host.PLANE_ZX, -30.0, -30.0, 30.0, 30.0, 0.0, host.Lambertian(host.SolidTexture(0.6, 0.6, 0.6))))
    side = int(math.ceil(math.sqrt(n)))
    for i in range(n):
        le = float(2.0 + (i * 7) % 11)
        tex = host.SolidTexture(le, 0.5 * le, 0.25 * le)
        if i % 5 == 4:
            tex = host.CheckerTexture(host.SolidTexture(3.0, 3.0, 3.0), host.SolidTexture(1.0, 2.0, 1.0))
        mat = host.DiffuseLight(tex)
        x, z = (i % side - (side - 1) / 2) * 1.5 + float(rng.uniform(-0.2, 0.2)), (i // side - (side - 1) / 2) * 1.5
        y = 2.0 + float(rng.uniform(0.0, 1.5))
        h = 0.1 + 0.05 * (i % 3)
        kind = i % 4
        if kind == 0:
            world.push(host.Rect(host.PLANE_ZX, z - h, x - h, z + h, x + 2 * h, y, mat))
        elif kind == 1:
            world.push(host.Sphere((x, y, z), h, mat))
        elif kind == 2:
            world.push(host.Rect(host.PLANE_XY, x - h, y - h, x + h, y + h, z, mat))
        else:
            world.push(host.Rect(host.PLANE_YZ, y - h, z - 2 * h, y + h, z + h, x, mat))
    return world


def spheres_in_a_tree(host):
    """five emissive and three plain spheres in one refittable BVH item, over a floor"""
    host.seed_scene_rng(3)
    world = host.HittableList()
    world.push(host.Rect(host.PLANE_ZX, -30.0, -30.0, 30.0, 30.0, 0.0, host.Lambertian(host.SolidTexture(0.6, 0.6, 0.6))))
    members = []
    for i in range(8):
        le = 3.0 + i
        mat = host.DiffuseLight(host.SolidTexture(le, le, 0.5 * le)) if i in (0, 2, 3, 5, 6) else host.Lambertian(host.SolidTexture(0.5, 0.4, 0.3))
        members.append(host.Sphere((-3.5 + i, 1.0 + 0.25 * (i % 3), 0.5 * (i % 2)), 0.3 + 0.02 * i, mat))
    world.push(host.BVHNode(members, 0.0, 1.0))
    return world


def table_of(scene):
    """the light table and the tree of a lowered scene's description: (lights LIGHT [n], nodes, paths)"""
    lights = scene.lights().astype(LIGHT)
    nodes, paths = scene.light_tree()
    return lights, nodes, paths


def moved_planes(arr, lights, seed, amount=0.4):
    """new planes A, B: every listed light shifted by a random offset and scaled a little, everything else as it is"""
    rng = np.random.default_rng(seed)
    a, b = arr["prim_a"].copy(), arr["prim_b"].copy()
    for L in lights:
        p = int(L["prim"])
        d = rng.uniform(-amount, amount, 3).astype(np.float32)
        s = np.float32(rng.uniform(0.8, 1.25))
        if L["kind"] == abi.PRIM_RECT:
            plane = (int(arr["prim_meta"][p]["flags"]) >> PLANE_SHIFT) & 3
            ka, kb, kk = ((1, 2, 0), (2, 0, 1), (0, 1, 2))[plane]
            a0, b0, a1, b1 = a[p]
            a[p] = (a0 + d[ka], b0 + d[kb], a0 + d[ka] + (a1 - a0) * s, b0 + d[kb] + (b1 - b0) * s)
            b[p, 0] += d[kk]
        else:
            a[p, :3] += d
            a[p, 3] *= s
    return a, b


def relight(d_arr, base, lights, nodes):
    """rtml_relight_desc on copies -> (rc, lights, nodes)"""
    lights = lights.copy()
    nodes = None if nodes is None else nodes.copy()
    d = R.to_desc(d_arr, base)
    rc = abi.load_rtmi().rtml_relight_desc(C.byref(d), lights.ctypes.data_as(C.POINTER(abi.Light)), len(lights),
                                           nodes.ctypes.data if nodes is not None and len(nodes) else None, 0 if nodes is None else len(nodes))
    return rc, lights, nodes


def restate(arr, lights, nodes):
    """the rules with explicit loops -> (lights, nodes)"""
    lights = lights.copy()
    n = len(lights)
    A, B, meta = arr["prim_a"], arr["prim_b"], arr["prim_meta"]
    aw, planes = [], []
    total = f64(0.0)
    for i in range(n):
        p = int(lights[i]["prim"])
        a = [f64(v) for v in A[p]]
        if lights[i]["kind"] == abi.PRIM_RECT:
            planes.append((int(meta[p]["flags"]) >> PLANE_SHIFT) & 3)
            area = (a[2] - a[0]) * (a[3] - a[1])
        else:
            planes.append(-1)
            area = ((f64(4.0) * f64(math.pi)) * a[3]) * a[3]
        lights[i]["area"] = area
        aw.append(area * f64(lights[i]["weight"]))
        total = total + aw[i]
    c = f64(0.0)
    for i in range(n):
        sp = aw[i] / total
        lights[i]["select_p"] = sp
        c = c + sp
        lights[i]["cdf"] = 1.0 if i + 1 == n else c
    if nodes is None or len(nodes) == 0:
        return lights, nodes
    nodes = nodes.copy()
    lo, hi, pw = {}, {}, {}
    mn = lambda x, y: y if y < x else x  # noqa: E731
    mx = lambda x, y: y if y > x else x  # noqa: E731
    for s in range(len(nodes) - 1, 0, -1):
        link = int(nodes[s]["link"])
        if link & LEAF:
            li = link & 0x7FFFFFFF
            p = int(lights[li]["prim"])
            a = [f64(v) for v in A[p]]
            if planes[li] >= 0:
                ka, kb, kk = ((1, 2, 0), (2, 0, 1), (0, 1, 2))[planes[li]]
                l3, h3 = [None] * 3, [None] * 3
                l3[ka], h3[ka], l3[kb], h3[kb] = a[0], a[2], a[1], a[3]
                l3[kk] = h3[kk] = f64(B[p][0])
            else:
                l3, h3 = [a[k] - a[3] for k in range(3)], [a[k] + a[3] for k in range(3)]
            lo[s], hi[s], pw[s] = l3, h3, aw[li]
        else:
            lo[s] = [mn(lo[link][k], lo[link + 1][k]) for k in range(3)]
            hi[s] = [mx(hi[link][k], hi[link + 1][k]) for k in range(3)]
            pw[s] = pw[link] + pw[link + 1]
        h = [(hi[s][k] - lo[s][k]) * f64(0.5) for k in range(3)]
        nodes[s]["c"] = [np.float32((lo[s][k] + hi[s][k]) * f64(0.5)) for k in range(3)]
        nodes[s]["r2"] = np.float32((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
        nodes[s]["power"] = np.float32(pw[s])
    return lights, nodes


def device_table(arr, lights):
    """what rtmi_scene_attach_lights uploads for a table: DEV_LIGHT [n] and the per-primitive light index"""
    out = np.zeros(len(lights), DEV_LIGHT)
    prim_light = np.full(len(arr["prim_a"]), -1, np.int32)
    for i, L in enumerate(lights):
        p = int(L["prim"])
        out[i]["geo"] = arr["prim_a"][p]
        out[i]["k"] = arr["prim_b"][p][0]
        out[i]["plane"] = ((int(arr["prim_meta"][p]["flags"]) >> PLANE_SHIFT) & 3) if L["kind"] == abi.PRIM_RECT else -1
        out[i]["item"], out[i]["prim"] = L["item"], p
        out[i]["area"], out[i]["p_sel"], out[i]["cdf"] = np.float32(L["area"]), np.float32(L["select_p"]), np.float32(L["cdf"])
        prim_light[p] = i
    return out, prim_light


assert LIGHT_NODE_DTYPE.itemsize == 32 and LIGHT.itemsize == 48 and DEV_LIGHT.itemsize == 48


def lights_of(arr, base):
    """rtmi_lights_from_desc of the description `base` with the arrays `arr`"""
    lib, d, n = abi.load_rtmi(), R.to_desc(arr, base), C.c_uint32(0)
    assert lib.rtmi_lights_from_desc(C.byref(d), None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, LIGHT)
    assert lib.rtmi_lights_from_desc(C.byref(d), out.ctypes.data_as(C.POINTER(abi.Light)), n.value, C.byref(n)) == 0
    return out


def last_error():
    return (abi.load_rtmi().rtmi_last_error() or b"").decode()
