"""What the oracle tests of the environment estimator and of roulette share (include/rtmi_env.h, include/rtmi_roulette.h):
maps that reach the lookup's and the sampler's edges, two hand-built scenes, and the light table of a scene
for the oracle.  numpy only; no GPU."""
import functools

import numpy as np

import env_ref
import scenes_extra
from nee_oracle_ref import oracle_lights
from oracle.oracle import LIGHT_DTYPE
from raytracing_rust_amd import scenes


def build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


# ---- maps -------------------------------------------------------------------------------------------------------------------
def zero_rows_map():
    """24 x 12, runs of all-zero rows at the top, in the middle and at the bottom.  The texel weight takes the largest
    channel over 3 x 3 texels, so only the inner rows of a run (0, 1, 6, 7, 11) have R[j] = 0: col_p = 0, col_cdf = 1, and
    a BSDF ray that leaves the world through one of them has pdf = 0 (weight 1)."""
    rng = np.random.default_rng(5)
    m = (rng.random((12, 24, 3)) * 3.0).astype(np.float32)
    m[[0, 1, 2, 5, 6, 7, 8, 10, 11]] = 0.0
    return m


def poles_map():
    """2 x 16384 (the largest height): a dim sky, bright only in the top and the bottom row, which with their neighbours
    (the texel weight looks one row further) take about 2/3 of the light samples.  Rows are pi / 16384 high, so those
    samples aim within 4e-4 of the poles, where ct -> 0: fy within ~5e-4 of the row's outer edge rounds v to exactly 1 or
    0, theta to +-RTMI_PIO2_F, and rtmi_cosf of that is negative: no sample."""
    m = np.full((16384, 2, 3), 2.0e-3, np.float32)
    m[0] = np.float32([6.0e4, 5.0e4, 4.0e4])
    m[-1] = np.float32([1.0e4, 2.0e4, 3.0e4])
    return m


def seam_map():
    """8 x 4, dim but for two different bright texels in column 0 and column W - 1 of one row: a lookup left of the
    centre of column 0 or right of the centre of column W - 1 (the phi = +-pi seam) interpolates across the wrap."""
    m = np.full((4, 8, 3), 0.02, np.float32)
    m[1, 0] = np.float32([30.0, 20.0, 10.0])
    m[1, 7] = np.float32([5.0, 15.0, 40.0])
    return m


@functools.lru_cache(maxsize=None)
def maps():
    """name -> float32 [H, W, 3]: the maps of tests/test_gpu_env.py (1x1, 3x2, 64x32, sun, zero) and the three above."""
    from test_gpu_env import _maps

    m = {k: v for k, v in _maps().items() if k != "earth"}
    m.update({"zero_rows": zero_rows_map(), "poles": poles_map(), "seam": seam_map()})
    return m


# ---- scenes (backend-agnostic: host or oracle `api`) ---------------------------------------------------------------------------
def well(api, nx, ny, lid=False, albedo=0.7):
    """A Lambertian shaft, 2 x 6 x 2, normals turned inward, seen from inside near its open top looking down: paths make
    many diffuse vertices before they leave through the opening.  lid=True closes it: every shadow ray toward a map is
    occluded and every camera path ends inside, at the depth limit."""
    mat = api.Lambertian(api.SolidTexture(albedo, 0.9 * albedo, 0.8 * albedo))
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_YZ, 0.0, -1.0, 6.0, 1.0, -1.0, mat))
    w.push(api.FlipNormals(api.Rect(api.PLANE_YZ, 0.0, -1.0, 6.0, 1.0, 1.0, mat)))
    w.push(api.Rect(api.PLANE_XY, -1.0, 0.0, 1.0, 6.0, -1.0, mat))
    w.push(api.FlipNormals(api.Rect(api.PLANE_XY, -1.0, 0.0, 1.0, 6.0, 1.0, mat)))
    w.push(api.Rect(api.PLANE_ZX, -1.0, -1.0, 1.0, 1.0, 0.0, mat))
    if lid:
        w.push(api.FlipNormals(api.Rect(api.PLANE_ZX, -1.0, -1.0, 1.0, 1.0, 6.0, mat)))
    cam = api.Camera((0.3, 5.5, 0.2), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 60.0, nx / ny, 0.0, 1.0, 0.0, 1.0)
    return cam, w


def black_room(api, nx, ny):
    """roulette_ref's open box with a black Lambertian sphere and a black cube in it: a scatter off either sets T to
    exactly 0, and the roulette test ends that continuation by m == 0, without a draw."""
    grey = api.Lambertian(api.SolidTexture(0.6, 0.6, 0.6))
    black = api.Lambertian(api.SolidTexture(0.0, 0.0, 0.0))
    lamp = api.DiffuseLight(api.SolidTexture(12.0, 12.0, 12.0))
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_YZ, 0.0, 0.0, 10.0, 10.0, 0.0, grey))
    w.push(api.FlipNormals(api.Rect(api.PLANE_YZ, 0.0, 0.0, 10.0, 10.0, 10.0, grey)))
    w.push(api.Rect(api.PLANE_ZX, 0.0, 0.0, 10.0, 10.0, 0.0, grey))
    w.push(api.FlipNormals(api.Rect(api.PLANE_ZX, 0.0, 0.0, 10.0, 10.0, 10.0, grey)))
    w.push(api.FlipNormals(api.Rect(api.PLANE_XY, 0.0, 0.0, 10.0, 10.0, 10.0, grey)))
    w.push(api.Rect(api.PLANE_ZX, 3.5, 3.5, 6.5, 6.5, 9.9, lamp))
    w.push(api.Sphere((3.0, 2.0, 6.0), 2.0, black))
    w.push(api.Cube((5.5, 0.0, 2.5), (8.5, 4.0, 5.5), black))
    cam = api.Camera((5.0, 5.0, -14.0), (5.0, 5.0, 10.0), (0.0, 1.0, 0.0), 40.0, nx / ny, 0.0, 10.0, 0.0, 1.0)
    return cam, w


# ---- light tables -----------------------------------------------------------------------------------------------------------
def lights_for(host, orc, world_h, world_o):
    """The oracle's light table of world_o in the order of the lowered world_h's (empty for a scene without lights), and
    the lowered scene."""
    sc = host.lower(world_h)
    if len(sc.lights()) == 0:
        assert not np.any(orc.emitters(world_o)["eligible"])
        return np.zeros(0, LIGHT_DTYPE), sc
    return oracle_lights(orc, world_o, sc), sc
