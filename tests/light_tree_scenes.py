"""Test-only scenes and point sets of the light tree (include/rtmi_light_tree.h), built with the backend-agnostic `api` of
raytracing_rust_amd.scenes: a floor under a grid of lamps, the degenerate tables (two lights at one place, powers 10^6
apart, one light, none) and a mix of rect and sphere lights."""
import numpy as np

import scenes_extra
from raytracing_rust_amd import scenes

ONE_MINUS = np.float32(1.0) - np.float32(2.0 ** -24)


def _floor(api, half=40.0, albedo=0.7):
    return api.Rect(api.PLANE_ZX, -half, -half, half, half, 0.0, api.Lambertian(api.SolidTexture(albedo, albedo, albedo)))


def _lamp(api, cx, cz, le, y=1.0, half=0.1):
    return api.Rect(api.PLANE_ZX, cz - half, cx - half, cz + half, cx + half, y, api.DiffuseLight(api.SolidTexture(le, le, le)))


def lamp_grid(api, g=16, bright_every=4, le=20.0):
    """g x g rect lamps of 0.2 x 0.2 at height 1, spacing 2, under a BVHNode, every bright_every-th lamp 5x brighter (0: all
    equal), over a Lambertian floor.  Height is z and the rects are XY ones: the reference gives every rect the bounding
    box of an XY rect (rect.rs:71-75, which the device reproduces), so a ZX lamp under a BVHNode is culled by a box that
    lies elsewhere and lights nothing; XY is the one orientation a BVHNode of rects can have."""
    lamps = []
    for i in range(g):
        for k in range(g):
            bright = bright_every and (i * g + k) % bright_every == bright_every - 1
            cx, cy = (i - (g - 1) / 2) * 2.0, (k - (g - 1) / 2) * 2.0
            e = 5.0 * le if bright else le
            lamps.append(api.Rect(api.PLANE_XY, cx - 0.1, cy - 0.1, cx + 0.1, cy + 0.1, 1.0, api.DiffuseLight(api.SolidTexture(e, e, e))))
    half = max(40.0, g * 1.5)
    world = api.HittableList()
    world.push(api.Rect(api.PLANE_XY, -half, -half, half, half, 0.0, api.Lambertian(api.SolidTexture(0.7, 0.7, 0.7))))
    world.push(api.BVHNode(lamps, 0.0, 1.0))
    return world


def lamp_grid_camera(api, nx, ny, g=16):
    """looks down on lamp_grid(g) from the side, z up"""
    look_from = (0.0, -24.0, 12.0) if g <= 16 else (0.0, -90.0, 30.0)
    return scenes.set_camera(api, nx, ny, look_from, (0.0, 0.0, 0.0), view_up=(0.0, 0.0, 1.0), vertical_fov=40.0)


def same_place(api):
    """two lights at the same place (the second hides behind the first from below), and a third elsewhere"""
    world = api.HittableList()
    world.push(_floor(api))
    world.push(_lamp(api, 1.0, 2.0, 3.0))
    world.push(_lamp(api, 1.0, 2.0, 5.0))
    world.push(_lamp(api, -3.0, 0.0, 4.0))
    return world


def far_powers(api):
    """powers 10^6 apart: a large bright rect and a dim speck"""
    world = api.HittableList()
    world.push(_floor(api))
    world.push(api.Rect(api.PLANE_ZX, -5.0, -5.0, 5.0, 5.0, 6.0, api.DiffuseLight(api.SolidTexture(100.0, 100.0, 100.0))))
    world.push(_lamp(api, 3.0, -2.0, 0.25, y=0.5))
    return world


def one_light(api):
    world = api.HittableList()
    world.push(_floor(api))
    world.push(_lamp(api, 0.5, -0.5, 8.0, y=2.0, half=0.5))
    return world


def no_light(api):
    world = api.HittableList()
    world.push(_floor(api))
    world.push(api.Sphere((0.0, 1.0, 0.0), 1.0, api.Lambertian(api.SolidTexture(0.4, 0.2, 0.1))))
    return world


def mixed(api):
    """rects in all three planes and spheres, at different heights, sizes and powers"""
    light = lambda le: api.DiffuseLight(api.SolidTexture(le, 0.5 * le, 0.25 * le))  # noqa: E731
    world = api.HittableList()
    world.push(_floor(api))
    world.push(api.Rect(api.PLANE_ZX, -1.0, -2.0, 1.5, 1.0, 3.0, light(4.0)))
    world.push(api.Rect(api.PLANE_XY, 2.0, 0.5, 3.0, 2.5, -4.0, light(2.0)))
    world.push(api.Rect(api.PLANE_YZ, 0.5, -1.0, 1.5, 1.0, 6.0, light(9.0)))
    world.push(api.Sphere((-4.0, 1.0, 2.0), 0.5, light(6.0)))
    world.push(api.Sphere((0.0, 5.0, -3.0), 1.25, light(1.0)))
    world.push(api.Sphere((5.0, 0.25, 5.0), 0.25, light(30.0)))
    world.push(api.Sphere((1.0, 0.5, -1.0), 0.5, api.Lambertian(api.SolidTexture(0.6, 0.6, 0.6))))
    return world


def four_rects(api, le, albedo):
    """four rect lights of radiance le at different heights and offsets over tests/test_gpu_nee.py's floor, none hiding
    another from the floor under its camera (|x|, |z| <= 0.27); returns the world and, per light, (corner, edge a, edge b)
    for nee_ref.f_rect"""
    spec = [(-1.0, -2.0, 1.5, 1.0, 3.0), (0.5, 0.75, 2.0, 2.25, 1.5), (-1.5, -0.5, -0.5, 0.5, 0.75), (-1.5, -6.5, 1.5, -4.5, 5.0)]
    world = api.HittableList()
    world.push(api.Rect(api.PLANE_ZX, -50.0, -50.0, 50.0, 50.0, 0.0, api.Lambertian(api.SolidTexture(albedo, albedo, albedo))))
    geo = []
    for z0, x0, z1, x1, h in spec:
        world.push(api.Rect(api.PLANE_ZX, z0, x0, z1, x1, h, api.DiffuseLight(api.SolidTexture(le, le, le))))
        geo.append((np.array([x0, h, z0]), np.array([0.0, 0.0, z1 - z0]), np.array([x1 - x0, 0.0, 0.0])))
    return world, geo


# name -> (world builder, look_from, look_at, vertical fov)
TREE_SCENES = {
    "lamp_grid": (lamp_grid, None, None, None),  # lamp_grid_camera
    "equal_lamps_4096": (lambda api: lamp_grid(api, 64, 0), None, None, None),
    "same_place": (same_place, (0.0, 6.0, -10.0), (0.0, 0.0, 0.0), 40.0),
    "far_powers": (far_powers, (0.0, 3.0, -12.0), (0.0, 0.0, 0.0), 40.0),
    "one_light": (one_light, (0.0, 3.0, -8.0), (0.0, 0.0, 0.0), 40.0),
    "no_light": (no_light, (0.0, 3.0, -8.0), (0.0, 0.0, 0.0), 40.0),
    "mixed": (mixed, (0.0, 5.0, -14.0), (0.0, 1.0, 0.0), 40.0),
}
REFERENCE_LIT = ["cornell_box", "lit_random_spheres", "lit_final_scene", "lit_smoke", "hollow_glass"]
WITH_LIGHTS = REFERENCE_LIT + [n for n in TREE_SCENES if n != "no_light"]


def build(api, name, nx, ny):
    """(camera, world) of a scene of this file, of tests/scenes_extra.py or of raytracing_rust_amd.scenes"""
    if name in TREE_SCENES:
        fn, look_from, look_at, vfov = TREE_SCENES[name]
        if look_from is None:
            return lamp_grid_camera(api, nx, ny, 16 if name == "lamp_grid" else 64), fn(api)
        return scenes.set_camera(api, nx, ny, look_from, look_at, vertical_fov=vfov), fn(api)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def probe_points(lo, hi, n=10240, seed=3):
    """n (x, u) pairs for a table with the light boxes lo, hi [lights, 3]: points around and far outside the lights' bounds,
    at lamp centres (d2 = 0 at a leaf), 10^6 away, and the uniforms 0 and 1 - 2^-24 among random 24-bit ones"""
    rng = np.random.default_rng(seed)
    blo, bhi = lo.min(0), hi.max(0)
    size = np.maximum(bhi - blo, 1.0)
    x = rng.uniform(blo - 0.75 * size, bhi + 0.75 * size, (n, 3))
    k = len(lo)
    cen = ((lo + hi) * 0.5)[rng.integers(0, k, 64)]
    x[:64] = cen
    x[64:128] = cen[:, :] + rng.normal(0.0, 1e-3, (64, 3)) * size
    x[128:136] = 1e6 * np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [-1, 1, -1]])
    u = (rng.integers(0, 1 << 24, n).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    u[0:n:7] = 0.0
    u[3:n:7] = ONE_MINUS
    return x.astype(np.float32), u
