"""ctypes binding of the CPU oracle (oracle/rt_oracle.c) — TEST INFRASTRUCTURE.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this
module.  The product package (raytracing_rust_amd/) never does.

The class exposes the reference's constructor names (Sphere, Rect, Lambertian, ...;
reference: src/*.rs `new` functions) so that the scene builders in
raytracing_rust_amd/scenes.py can be run against either backend.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "_build")

ARITH_DEVICE = 1
THROUGHPUT_FORM = 2
SKY = 4  # opt-in extension: gradient background of color.rs:18-20 (commented out in the reference)
FACE_FORWARD = 8  # opt-in extension: opaque materials scatter about the normal turned against the ray
UV_BOOK = 16  # opt-in extension: get_sphere_uv with pi/2 (the book) instead of FRAC_2_PI (sphere.rs:13)

COUNTER_NAMES = [
    "samples", "queries", "aabb", "sphere", "msphere", "rect", "xform", "medium", "medium_draw",
    "mat_fetch", "tex_solid", "tex_checker", "tex_noise", "tex_image", "sc_lambert", "sc_metal",
    "sc_dielectric", "sc_isotropic", "emit", "draws", "sphere_trials", "disk_trials", "sphere_accept",
    "rect_accept",
    # the environment estimator and roulette (appended: the indices above keep their meaning)
    "env_sample", "env_no_sample", "env_occluded", "env_unoccluded", "env_miss_mis", "env_miss_one", "env_area_sample",
    "env_emit_scaled", "rr_test", "rr_draw", "rr_end_pending", "rr_end_bare", "rr_floor_survive", "rr_zero",
    # the light tree under render_nee (appended)
    "tree_walk", "tree_left", "tree_right", "tree_floor", "tree_p_one", "tree_clamp", "tree_no_sample", "tree_hit_pmf",
    "tree_hit_picked", "tree_hit_picked_mismatch",
]
ENV_COUNTERS = COUNTER_NAMES[24:32]
ROULETTE_COUNTERS = COUNTER_NAMES[32:38]
TREE_COUNTERS = COUNTER_NAMES[38:48]
ROULETTE_ESTIMATORS = {"plain": 0, "nee": 1, "env": 2, "env_nee": 3}  # RTMI_ROULETTE_*

PLANE_YZ, PLANE_ZX, PLANE_XY = 0, 1, 2

# next-event estimation (include/rtmi_nee.h): kinds as RTMI_PRIM_SPHERE / RTMI_PRIM_RECT; geo = rect {a0, b0, a1, b1, k},
# sphere {cx, cy, cz, r, 0}
KIND_SPHERE, KIND_RECT = 0, 2
EMITTER_DTYPE = np.dtype([("handle", "<u8"), ("kind", "<i4"), ("plane", "<i4"), ("geo", "<f8", (5,)),
                          ("under_xform", "<i4"), ("in_medium", "<i4"), ("count", "<i4"), ("eligible", "<i4"),
                          ("weight", "<f8"), ("area", "<f8")])  # OrcEmitter, 88 B
LIGHT_DTYPE = np.dtype([("handle", "<u8"), ("kind", "<i4"), ("plane", "<i4"), ("geo", "<f8", (5,)), ("area", "<f8"),
                        ("p_sel", "<f8"), ("cdf", "<f8")])  # OrcLight, 80 B
# the light tree (include/rtmi_light_tree.h): rtmi_light_node and rtmi_light_path as the oracle reads them
LIGHT_NODE_DTYPE = np.dtype([("c", "<f4", (3,)), ("r2", "<f4"), ("power", "<f4"), ("link", "<u4"), ("pad", "<u4", (2,))])  # 32 B
LIGHT_PATH_DTYPE = np.dtype([("trail", "<u4"), ("depth", "<u4")])  # 8 B
AXIS_X, AXIS_Y, AXIS_Z = 0, 1, 2


class OrcEnv(C.Structure):
    """The map and its sampling tables as orc_render_env takes them (OrcEnv, 56 B)."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("rgb", C.c_void_p), ("row_cdf", C.c_void_p), ("row_p", C.c_void_p),
                ("col_cdf", C.c_void_p), ("col_p", C.c_void_p), ("total", C.c_double)]


def _env(env_rgb, tables):
    """(OrcEnv, the arrays it points into) of a float32 [H, W, 3] map and its tables: a dict with row_cdf [H], row_p [H],
    col_cdf [H, W], col_p [H, W] (float32) and total (float), as include/rtmi_env.h's rtmi_env_tables writes them."""
    rgb = np.ascontiguousarray(env_rgb, dtype=np.float32)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    keep = [rgb]
    for k, shape in (("row_cdf", (h,)), ("row_p", (h,)), ("col_cdf", (h, w)), ("col_p", (h, w))):
        a = np.ascontiguousarray(tables[k], dtype=np.float32)
        assert a.shape == shape, (k, a.shape)
        keep.append(a)
    return OrcEnv(w, h, *[a.ctypes.data for a in keep], float(tables["total"])), keep


def _tree(tree):
    """(nodes, paths) of a light tree as contiguous arrays of the oracle's own dtypes; the bytes are taken as they are"""
    nodes, paths = (np.ascontiguousarray(a) for a in tree)
    assert nodes.dtype.itemsize == LIGHT_NODE_DTYPE.itemsize and paths.dtype.itemsize == LIGHT_PATH_DTYPE.itemsize
    return nodes.view(LIGHT_NODE_DTYPE), paths.view(LIGHT_PATH_DTYPE)


def build():
    """Compile both oracle libraries (gcc, a few seconds)."""
    subprocess.run(["make", "-C", _HERE, "all"], check=True, stdout=subprocess.DEVNULL)


_NATIVE_BUILT = False


def build_native():
    """The timed CPU-baseline library: no counters, -march=native.  Rebuilt once per process tree on the host
    that runs it (the file may have been compiled on another host); forked workers inherit the flag."""
    global _NATIVE_BUILT
    if not _NATIVE_BUILT:
        subprocess.run(["make", "-B", "-C", _HERE, "native"], check=True, stdout=subprocess.DEVNULL)
        _NATIVE_BUILT = True


def _load(name):
    path = os.path.join(_BUILD, name)
    if name == "liborc_f64_native.so":
        build_native()
    elif not os.path.exists(path):
        build()
    lib = C.CDLL(path)
    vp, d, i, u64 = C.c_void_p, C.c_double, C.c_int, C.c_uint64
    sig = {
        "orc_is_f32": (i, []),
        "orc_set_flags": (None, [i]),
        "orc_seed_scene_rng": (None, [u64]),
        "orc_scene_uniform": (d, []),
        "orc_scene_range": (C.c_uint32, [C.c_uint32]),
        "orc_philox": (None, [vp, vp, vp]),
        "orc_free_all": (None, []),
        "orc_tex_solid": (vp, [d, d, d]),
        "orc_tex_checker": (vp, [vp, vp]),
        "orc_tex_noise": (vp, [d]),
        "orc_tex_image": (vp, [vp, C.c_uint32, C.c_uint32]),
        "orc_perlin_tables": (None, [vp, vp, vp]),
        "orc_mat_lambertian": (vp, [vp]),
        "orc_mat_metal": (vp, [vp, d]),
        "orc_mat_dielectric": (vp, [d]),
        "orc_mat_diffuse_light": (vp, [vp]),
        "orc_mat_isotropic": (vp, [vp]),
        "orc_sphere": (vp, [d, d, d, d, vp]),
        "orc_moving_sphere": (vp, [d] * 9 + [vp]),
        "orc_rect": (vp, [i, d, d, d, d, d, vp]),
        "orc_cube": (vp, [d] * 6 + [vp]),
        "orc_list_new": (vp, []),
        "orc_list_push": (None, [vp, vp]),
        "orc_flip_normals": (vp, [vp]),
        "orc_translate": (vp, [vp, d, d, d]),
        "orc_rotate": (vp, [i, vp, d]),
        "orc_constant_medium": (vp, [vp, d, vp]),
        "orc_bvh": (vp, [vp, i, d, d]),
        "orc_camera": (vp, [d] * 15),
        "orc_camera_state": (None, [vp, vp]),
        "orc_render": (i, [vp, vp, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp]),
        "orc_render_samples": (i, [vp, vp, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp, vp]),
        "orc_render_nee": (i, [vp, vp, vp, i, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp, vp]),
        "orc_render_nee_tree": (i, [vp, vp, vp, i, vp, i, vp, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp, vp]),
        "orc_light_tree_pick": (i, [vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp]),
        "orc_light_tree_pmf": (i, [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]),
        "orc_render_env": (i, [vp, vp, vp, i, vp, i, d, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp, vp]),
        "orc_render_roulette": (i, [vp, vp, vp, i, vp, i, i, d, d, i, i, i, u64, i, i, d, i, i, vp, vp, vp, vp, vp, vp]),
        "orc_env_lookup": (i, [vp, d, i, vp, vp, C.c_long]),
        "orc_env_sample": (i, [vp, d, i, vp, vp, C.c_long]),
        "orc_emitters": (i, [vp, vp, i]),
        "orc_ppm_text": (C.c_size_t, [i, i, vp, vp, C.c_size_t]),
        "orc_hit": (i, [vp, vp, vp, d, d, d, i, u64, vp, vp]),
        "orc_bounding_box": (i, [vp, d, d, vp]),
        "orc_tex_value": (None, [vp, d, d, vp, i, vp]),
        "orc_scatter": (i, [vp, vp, vp, d, vp, i, u64, vp]),
        "orc_emitted": (None, [vp, d, d, vp, vp]),
        "orc_get_ray": (None, [vp, d, d, u64, vp]),
        "orc_reset_counters": (None, []),
        "orc_get_counters": (i, [vp, i]),
        "orc_rtmi_sinf": (C.c_float, [C.c_float]),
        "orc_rtmi_cosf": (C.c_float, [C.c_float]),
        "orc_rtmi_logf": (C.c_float, [C.c_float]),
        "orc_rtmi_atan2f": (C.c_float, [C.c_float, C.c_float]),
        "orc_rtmi_asinf": (C.c_float, [C.c_float]),
        "orc_probe_aabb": (i, [vp, vp, vp, d, d, i]),
        "orc_probe_medium": (None, [vp, vp, vp, d, i, vp]),
        "orc_probe_shade": (None, [vp, vp, d, d, d, vp]),
        "orc_probe_uv": (None, [vp, i, vp]),
        "orc_script": (None, [vp, C.c_uint32]),
        "orc_script_consumed": (C.c_uint32, []),
        "orc_sample_unit": (None, [i, vp]),
        "orc_sample_unit_wrong": (None, [i, d, vp]),
        "orc_medium_sample": (i, [d, d, d, d, d, d, i, vp]),
        "orc_pixel_ray": (None, [vp, i, i, i, i, vp]),
        "orc_camera_from_state": (vp, [vp]),
        "orc_probe_point": (vp, [d, d, d, d]),
        "orc_bounce": (None, [vp, vp, vp, d, d, d, i, i, i, vp]),
    }
    for name_, (res, args) in sig.items():
        fn = getattr(lib, name_)
        fn.restype = res
        fn.argtypes = args
    return lib


class _Obj:
    """Opaque handle to an oracle object (lives until Oracle.free_all())."""

    __slots__ = ("h", "keep")

    def __init__(self, h, keep=()):
        if not h:
            raise RuntimeError("oracle constructor failed (reference would panic here)")
        self.h = h
        self.keep = keep


class _List(_Obj):
    def push(self, hittable):
        self.keep = self.keep + (hittable,)
        self._lib.orc_list_push(self.h, hittable.h)


def _d3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3))


class Oracle:
    """One precision build of the oracle.  precision = 'f64' (literal) or 'f32'."""

    PLANE_YZ, PLANE_ZX, PLANE_XY = PLANE_YZ, PLANE_ZX, PLANE_XY
    AXIS_X, AXIS_Y, AXIS_Z = AXIS_X, AXIS_Y, AXIS_Z

    def __init__(self, precision="f64", native=False):
        """native=True: the uninstrumented -march=native f64 build that bench.py times as the CPU baseline."""
        assert precision in ("f64", "f32")
        assert not native or precision == "f64"
        self.precision = precision
        self.lib = _load("liborc_f64_native.so" if native else "liborc_%s.so" % precision)
        assert self.lib.orc_is_f32() == (1 if precision == "f32" else 0)

    # ---- scene RNG (the reference's thread_rng during construction) ----
    def seed_scene_rng(self, seed):
        self.lib.orc_seed_scene_rng(int(seed))

    def free_all(self):
        self.lib.orc_free_all()

    # ---- textures (src/texture.rs) ----
    def SolidTexture(self, r, g, b):
        return _Obj(self.lib.orc_tex_solid(r, g, b))

    def CheckerTexture(self, odd, even):
        return _Obj(self.lib.orc_tex_checker(odd.h, even.h), (odd, even))

    def NoiseTexture(self, scale):
        return _Obj(self.lib.orc_tex_noise(scale))

    def ImageTexture(self, data, nx, ny):
        arr = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1))
        assert arr.size == nx * ny * 3
        return _Obj(self.lib.orc_tex_image(arr.ctypes.data, nx, ny))

    # ---- materials (src/material.rs) ----
    def Lambertian(self, tex):
        return _Obj(self.lib.orc_mat_lambertian(tex.h), (tex,))

    def Metal(self, tex, fuzz):
        return _Obj(self.lib.orc_mat_metal(tex.h, fuzz), (tex,))

    def Dielectric(self, ref_idx):
        return _Obj(self.lib.orc_mat_dielectric(ref_idx))

    def DiffuseLight(self, tex):
        return _Obj(self.lib.orc_mat_diffuse_light(tex.h), (tex,))

    def Isotropic(self, tex):
        return _Obj(self.lib.orc_mat_isotropic(tex.h), (tex,))

    # ---- hittables ----
    def Sphere(self, center, radius, material):
        c = _d3(center)
        return _Obj(self.lib.orc_sphere(c[0], c[1], c[2], radius, material.h), (material,))

    def MovingSphere(self, center0, center1, time0, time1, radius, material):
        a, b = _d3(center0), _d3(center1)
        return _Obj(self.lib.orc_moving_sphere(a[0], a[1], a[2], b[0], b[1], b[2], time0, time1, radius,
                                               material.h), (material,))

    def Rect(self, plane, x0, y0, x1, y1, k, material):
        return _Obj(self.lib.orc_rect(plane, x0, y0, x1, y1, k, material.h), (material,))

    def Cube(self, p_min, p_max, material):
        a, b = _d3(p_min), _d3(p_max)
        return _Obj(self.lib.orc_cube(a[0], a[1], a[2], b[0], b[1], b[2], material.h), (material,))

    def FlipNormals(self, hittable):
        return _Obj(self.lib.orc_flip_normals(hittable.h), (hittable,))

    def Traslate(self, hittable, offset):
        o = _d3(offset)
        return _Obj(self.lib.orc_translate(hittable.h, o[0], o[1], o[2]), (hittable,))

    def Rotate(self, axis, hittable, angle):
        return _Obj(self.lib.orc_rotate(axis, hittable.h, angle), (hittable,))

    def ConstantMedium(self, boundary, density, texture):
        return _Obj(self.lib.orc_constant_medium(boundary.h, density, texture.h), (boundary, texture))

    def HittableList(self):
        l = _List(self.lib.orc_list_new())
        l._lib = self.lib
        return l

    def BVHNode(self, hittables, time0, time1):
        arr = (C.c_void_p * len(hittables))(*[h.h for h in hittables])
        return _Obj(self.lib.orc_bvh(arr, len(hittables), time0, time1), tuple(hittables))

    def Camera(self, look_from, look_at, view_up, vertical_fov, aspect, aperture, focus_dist, time0, time1):
        f, a, u = _d3(look_from), _d3(look_at), _d3(view_up)
        return _Obj(self.lib.orc_camera(f[0], f[1], f[2], a[0], a[1], a[2], u[0], u[1], u[2], vertical_fov, aspect,
                                        aperture, focus_dist, time0, time1))

    # ---- the hot path ----
    def render(self, cam, world, nx, ny, ns, seed=42, flags=0, max_depth=50, t_min=0.001, rows=None):
        """create_image (tests/test.rs:55-85).  Returns dict(linear f32 [ny,nx,3],
        rgb int32 [ny,nx,3], mean f64 [ny,nx,3], sig u64 [ny,nx] path signatures); row 0 is the top row."""
        r0, r1 = (0, ny) if rows is None else rows
        lin = np.zeros((ny, nx, 3), np.float32)
        rgb = np.zeros((ny, nx, 3), np.int32)
        mean = np.zeros((ny, nx, 3), np.float64)
        sig = np.zeros((ny, nx), np.uint64)
        rc = self.lib.orc_render(cam.h, world.h, nx, ny, ns, int(seed), flags, max_depth, t_min, r0, r1,
                                 lin.ctypes.data, rgb.ctypes.data, mean.ctypes.data, sig.ctypes.data)
        if rc != 0:
            raise RuntimeError("orc_render failed")
        return {"linear": lin, "rgb": rgb, "mean": mean, "sig": sig}

    def _outputs(self, nx, ny, ns, samples):
        out = {"linear": np.zeros((ny, nx, 3), np.float32), "rgb": np.zeros((ny, nx, 3), np.int32),
               "mean": np.zeros((ny, nx, 3), np.float64), "sig": np.zeros((ny, nx), np.uint64)}
        if samples:
            out["samples"] = np.zeros((ny, nx, ns, 3), np.float32)
        ptrs = [out[k].ctypes.data for k in ("linear", "rgb", "mean", "sig")] + [out["samples"].ctypes.data if samples else None]
        return out, ptrs

    def render_samples(self, cam, world, nx, ny, ns, seed=42, flags=0, max_depth=50, t_min=0.001, rows=None):
        """render() plus samples f32 [ny,nx,ns,3]: every sample's radiance as the fp32 value the device stores."""
        r0, r1 = (0, ny) if rows is None else rows
        out, ptrs = self._outputs(nx, ny, ns, True)
        if self.lib.orc_render_samples(cam.h, world.h, nx, ny, ns, int(seed), flags, max_depth, t_min, r0, r1, *ptrs) != 0:
            raise RuntimeError("orc_render_samples failed")
        return out

    def emitters(self, world):
        """Every DiffuseLight rect or sphere leaf of the graph (EMITTER_DTYPE), in the order the graph first reaches
        them: handle, kind, plane, geo, under_xform, in_medium, count (occurrences), weight, area, and whether it is
        eligible as a light under include/rtmi_nee.h's rules."""
        n = self.lib.orc_emitters(world.h, None, 0)
        out = np.zeros(max(n, 1), EMITTER_DTYPE)
        assert self.lib.orc_emitters(world.h, out.ctypes.data, n) == n
        return out[:n]

    def render_nee(self, cam, world, lights, nx, ny, ns, seed=42, flags=0, max_depth=50, t_min=0.001, rows=None,
                   samples=False, tree=None):
        """rtmi_render_nee's estimator (include/rtmi_nee.h) with the light table `lights` (LIGHT_DTYPE, the device's
        order; area, p_sel and cdf as the device's floats).  tree=(nodes, paths) (LIGHT_NODE_DTYPE, LIGHT_PATH_DTYPE; the
        tree over that table): the estimator under RTMI_FLAG_LIGHT_TREE (include/rtmi_light_tree.h).  Returns render()'s
        dict (the throughput form is implied), plus samples f32 [ny,nx,ns,3] when samples=True."""
        r0, r1 = (0, ny) if rows is None else rows
        lt = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        out, ptrs = self._outputs(nx, ny, ns, samples)
        if tree is None:
            rc = self.lib.orc_render_nee(cam.h, world.h, lt.ctypes.data if len(lt) else None, len(lt), nx, ny, ns, int(seed),
                                         flags, max_depth, t_min, r0, r1, *ptrs)
        else:
            nodes, paths = _tree(tree)
            rc = self.lib.orc_render_nee_tree(cam.h, world.h, lt.ctypes.data if len(lt) else None, len(lt),
                                              nodes.ctypes.data if len(nodes) else None, len(nodes),
                                              paths.ctypes.data if len(paths) else None, nx, ny, ns, int(seed), flags, max_depth,
                                              t_min, r0, r1, *ptrs)
        if rc != 0:
            raise RuntimeError("orc_render_nee failed")
        return out

    def light_tree_pick(self, nodes, points, us):
        """The walk of include/rtmi_light_tree.h from float32 points [n, 3] with the uniforms us [n] -> (light uint32 [n],
        probability float32 [n]); in this library's precision, the probability rounded to float."""
        nodes, _ = _tree((nodes, np.zeros(0, LIGHT_PATH_DTYPE)))
        x, u = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(us, np.float32)
        assert x.shape == (len(u), 3)
        light, p = np.zeros(len(u), np.uint32), np.zeros(len(u), np.float32)
        if self.lib.orc_light_tree_pick(nodes.ctypes.data, len(nodes), x.ctypes.data, u.ctypes.data, len(u), light.ctypes.data,
                                        p.ctypes.data) != 0:
            raise RuntimeError("orc_light_tree_pick failed")
        return light, p

    def light_tree_pmf(self, nodes, paths, points, lights):
        """The reverse walk: the probability float32 [n] that the walk from points [n, 3] ends at lights [n]."""
        nodes, paths = _tree((nodes, paths))
        x, li = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(lights, np.uint32)
        assert x.shape == (len(li), 3)
        p = np.zeros(len(li), np.float32)
        if self.lib.orc_light_tree_pmf(nodes.ctypes.data, len(nodes), paths.ctypes.data, x.ctypes.data, li.ctypes.data, len(li),
                                       p.ctypes.data) != 0:
            raise RuntimeError("orc_light_tree_pmf failed")
        return p

    def render_env(self, cam, world, lights, env_rgb, tables, nee, env_select_p, nx, ny, ns, seed=42, flags=0, max_depth=50,
                   t_min=0.001, rows=None, samples=False):
        """rtmi_render_env's estimator (include/rtmi_env.h): render_nee's arguments plus the map env_rgb (float32
        [H, W, 3]), its sampling tables (see _env), nee (False / True) and env_select_p.  p_env follows the header: env_select_p
        with a light table that is not empty, 1 with an empty one, 0 when tables["total"] is 0.  Returns render_nee's dict."""
        r0, r1 = (0, ny) if rows is None else rows
        lt = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        e, _keep = _env(env_rgb, tables)
        out, ptrs = self._outputs(nx, ny, ns, samples)
        rc = self.lib.orc_render_env(cam.h, world.h, lt.ctypes.data if len(lt) else None, len(lt), C.byref(e), 1 if nee else 0,
                                     float(env_select_p), nx, ny, ns, int(seed), flags, max_depth, t_min, r0, r1, *ptrs)
        if rc != 0:
            raise RuntimeError("orc_render_env failed")
        return out

    def render_roulette(self, cam, world, lights, env_rgb, tables, estimator, min_depth, q_min, env_select_p, nx, ny, ns,
                        seed=42, flags=0, max_depth=50, t_min=0.001, rows=None, samples=False):
        """rtmi_render_roulette's estimator (include/rtmi_roulette.h): estimator "plain", "nee", "env" or "env_nee" with
        the test from depth min_depth on and the floor q_min.  lights is read by "nee" and "env_nee", env_rgb and tables
        (None otherwise) by "env" and "env_nee".  Returns render_nee's dict plus bounces u32 [ny, nx]: the sum over the
        pixel's samples of the depth at which the path was written.  The throughput form is implied."""
        r0, r1 = (0, ny) if rows is None else rows
        est = ROULETTE_ESTIMATORS[estimator]
        lt = np.ascontiguousarray(lights if lights is not None else [], dtype=LIGHT_DTYPE)
        e, _keep = _env(env_rgb, tables) if est >= 2 else (None, None)
        out, ptrs = self._outputs(nx, ny, ns, samples)
        out["bounces"] = np.zeros((ny, nx), np.uint32)
        rc = self.lib.orc_render_roulette(cam.h, world.h, lt.ctypes.data if len(lt) else None, len(lt),
                                          C.byref(e) if e is not None else None, est, int(min_depth), float(q_min),
                                          float(env_select_p), nx, ny, ns, int(seed), flags, max_depth, t_min, r0, r1, *ptrs,
                                          out["bounces"].ctypes.data)
        if rc != 0:
            raise RuntimeError("orc_render_roulette failed")
        return out

    def env_lookup(self, env_rgb, tables, dirs, p_env=1.0, flags=ARITH_DEVICE):
        """The oracle's env(d) and BSDF-side pdf of float32 directions [n, 3] -> float32 [n, 4] = r, g, b, pdf."""
        e, _keep = _env(env_rgb, tables)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        out = np.zeros((len(d), 4), np.float32)
        assert self.lib.orc_env_lookup(C.byref(e), float(p_env), flags, d.ctypes.data, out.ctypes.data, len(d)) == 0
        return out

    def env_sample(self, env_rgb, tables, u12, p_env=1.0, flags=ARITH_DEVICE):
        """The oracle's light sample of float32 uniforms [n, 2] -> float32 [n, 4] = direction, pdf (zeros: no sample)."""
        e, _keep = _env(env_rgb, tables)
        u = np.ascontiguousarray(u12, dtype=np.float32)
        out = np.zeros((len(u), 4), np.float32)
        assert self.lib.orc_env_sample(C.byref(e), float(p_env), flags, u.ctypes.data, out.ctypes.data, len(u)) == 0
        return out

    def ppm_text(self, rgb):
        ny, nx = rgb.shape[:2]
        rgb = np.ascontiguousarray(rgb, dtype=np.int32)
        need = self.lib.orc_ppm_text(nx, ny, rgb.ctypes.data, None, 0)
        buf = C.create_string_buffer(need)
        n = self.lib.orc_ppm_text(nx, ny, rgb.ctypes.data, buf, need)
        return buf.raw[:n]

    # ---- probes ----
    def hit(self, hittable, origin, direction, time=0.0, t_min=0.001, t_max=float("inf"), flags=0, seed=0):
        o, d = _d3(origin), _d3(direction)
        out = np.zeros(9)
        mk = C.c_int(-1)
        tmx = 1.8e308 if t_max == float("inf") else t_max
        tmn = -1.8e308 if t_min == -float("inf") else t_min
        ok = self.lib.orc_hit(hittable.h, o.ctypes.data, d.ctypes.data, time, tmn, tmx, flags, seed,
                              out.ctypes.data, C.byref(mk))
        if not ok:
            return None
        return {"t": out[0], "u": out[1], "v": out[2], "p": out[3:6].copy(), "normal": out[6:9].copy(),
                "mat_kind": mk.value}

    def aabb_hit(self, origin, direction, box, t_min, t_max, flags=0):
        """aabb.rs:31-44 on the ray's derived 1/d (t_min / t_max beyond +-1.7e308: the precision's +-MAX)"""
        o, d, b = _d3(origin), _d3(direction), np.ascontiguousarray(np.asarray(box, np.float64).reshape(6))
        return bool(self.lib.orc_probe_aabb(o.ctypes.data, d.ctypes.data, b.ctypes.data, t_min, t_max, flags))

    def medium_queries(self, boundary, origin, direction, time=0.0, flags=0):
        """ConstantMedium's two boundary queries (medium.rs:29-30): (h1, t1, h2, t2)"""
        o, d = _d3(origin), _d3(direction)
        out = np.zeros(4)
        self.lib.orc_probe_medium(boundary.h, o.ctypes.data, d.ctypes.data, time, flags, out.ctypes.data)
        return bool(out[0]), out[1], bool(out[2]), out[3]

    def shade(self, v, n, ni_over_nt, cosine, ref_idx):
        """material.rs:9-28: (reflect(v, n), refract ok, refracted vector, schlick(cosine, ref_idx))"""
        vv, nn = _d3(v), _d3(n)
        out = np.zeros(8)
        self.lib.orc_probe_shade(vv.ctypes.data, nn.ctypes.data, ni_over_nt, cosine, ref_idx, out.ctypes.data)
        return out[0:3].copy(), bool(out[3]), out[4:7].copy(), out[7]

    def sphere_uv(self, n, flags=0):
        """get_sphere_uv (sphere.rs:9-15) of a unit normal: (u, v)"""
        nn = _d3(n)
        out = np.zeros(2)
        self.lib.orc_probe_uv(nn.ctypes.data, flags, out.ctypes.data)
        return out[0], out[1]

    def bounding_box(self, hittable, t0=0.0, t1=1.0):
        out = np.zeros(6)
        if not self.lib.orc_bounding_box(hittable.h, t0, t1, out.ctypes.data):
            return None
        return out[:3].copy(), out[3:].copy()

    def tex_value(self, tex, u, v, p, flags=0):
        pp = _d3(p)
        out = np.zeros(3)
        self.lib.orc_tex_value(tex.h, u, v, pp.ctypes.data, flags, out.ctypes.data)
        return out

    def scatter(self, mat, ray_o, ray_d, time, rec, flags=0, seed=0):
        o, d = _d3(ray_o), _d3(ray_d)
        r9 = np.ascontiguousarray(np.concatenate([[rec["t"], rec["u"], rec["v"]], rec["p"], rec["normal"]]),
                                  dtype=np.float64)
        out = np.zeros(10)
        ok = self.lib.orc_scatter(mat.h, o.ctypes.data, d.ctypes.data, time, r9.ctypes.data, flags, seed,
                                  out.ctypes.data)
        if not ok:
            return None
        return {"o": out[0:3].copy(), "d": out[3:6].copy(), "time": out[6], "attenuation": out[7:10].copy()}

    def emitted(self, mat, u, v, p):
        pp = _d3(p)
        out = np.zeros(3)
        self.lib.orc_emitted(mat.h, u, v, pp.ctypes.data, out.ctypes.data)
        return out

    def get_ray(self, cam, s, t, seed=0):
        out = np.zeros(7)
        self.lib.orc_get_ray(cam.h, s, t, seed, out.ctypes.data)
        return out

    def camera_state(self, cam):
        out = np.zeros(21)
        self.lib.orc_camera_state(cam.h, out.ctypes.data)
        return out

    # ---- the scripted word source (tests/test_path_contract.py): every call below sets the script, runs and clears it ----
    def _scripted(self, words, call):
        """call() with the render path's stream reading `words` (uint32) instead of Philox: (its result, words consumed,
        exhausted: a draw went beyond the script and got 0x80000000)"""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        self.lib.orc_script(w.ctypes.data if len(w) else None, len(w))
        try:
            res = call()
            used = int(self.lib.orc_script_consumed()) if len(w) else 0
        finally:
            self.lib.orc_script(None, 0)
        return res, used, used > len(w)

    def sample_unit(self, kind, words, wrong=None):
        """random_in_unit_sphere (kind 0) / random_in_unit_disk (kind 1) over scripted words: (p, consumed, exhausted);
        wrong=limit: the negative control that accepts |p|^2 <= limit instead of |p|^2 < 1"""
        out = np.zeros(3)
        if wrong is None:
            call = lambda: self.lib.orc_sample_unit(kind, out.ctypes.data)  # noqa: E731
        else:
            call = lambda: self.lib.orc_sample_unit_wrong(kind, float(wrong), out.ctypes.data)  # noqa: E731
        _, used, exh = self._scripted(words, call)
        return out, used, exh

    def medium_sample(self, t1, t2, t_min, t_max, dn, density, words, flags=0):
        """ConstantMedium::hit after its two boundary queries (medium.rs:33-53): (taken, t, consumed, exhausted)"""
        t = C.c_double(0.0)
        tmx = 1.8e308 if t_max == float("inf") else t_max
        tmn = -1.8e308 if t_min == -float("inf") else t_min
        ok, used, exh = self._scripted(words, lambda: self.lib.orc_medium_sample(t1, t2, tmn, tmx, dn, density, flags, C.byref(t)))
        return bool(ok), t.value, used, exh

    def pixel_ray(self, cam, i, j, nx, ny, words):
        """sample 0 of pixel (i, j) as the render takes it (tests/test.rs:66-68): (o (3), d (3), time), consumed, exhausted"""
        out = np.zeros(7)
        _, used, exh = self._scripted(words, lambda: self.lib.orc_pixel_ray(cam.h, i, j, nx, ny, out.ctypes.data))
        return out, used, exh

    def bounce(self, world, origin, direction, time, t_min, t_max, depth, max_depth, words, flags=0):
        """one turn of color's loop for a path with T = 1, L = 0 at `depth` over scripted words: None without a hit, else
        dict(t, p, normal, mat_kind, scattered, o, d, T, L, consumed, exhausted)"""
        o, dd = _d3(origin), _d3(direction)
        out = np.zeros(22)
        tmx = 1.8e308 if t_max == float("inf") else t_max
        _, used, exh = self._scripted(words, lambda: self.lib.orc_bounce(world.h, o.ctypes.data, dd.ctypes.data, time, t_min, tmx,
                                                                         depth, max_depth, flags, out.ctypes.data))
        if not out[0]:
            return None
        return {"t": out[1], "p": out[2:5].copy(), "normal": out[5:8].copy(), "mat_kind": int(out[8]), "scattered": bool(out[9]),
                "o": out[10:13].copy(), "d": out[13:16].copy(), "T": out[16:19].copy(), "L": out[19:22].copy(),
                "consumed": used, "exhausted": exh}

    def ProbePoint(self, t, normal):
        """test only: a hittable that reports a hit at parameter t with the given normal, whatever the ray; wrapped in
        Traslate / Rotate, Oracle.hit returns the chain's round trip of that point"""
        n = _d3(normal)
        return _Obj(self.lib.orc_probe_point(t, n[0], n[1], n[2]))

    def CameraFromState(self, state21):
        """a camera from its 21 derived values (origin, lower_left_corner, horizontal, vertical, u, v, time0, time1, lens_radius)"""
        s = np.ascontiguousarray(state21, dtype=np.float64).reshape(21)
        return _Obj(self.lib.orc_camera_from_state(s.ctypes.data))

    def perlin_tables(self, tex):
        rv = np.zeros(768)
        pm = np.zeros(768, np.int32)
        self.lib.orc_perlin_tables(tex.h, rv.ctypes.data, pm.ctypes.data)
        return rv.reshape(256, 3), pm.reshape(3, 256)

    def philox(self, ctr, key):
        c = np.asarray(ctr, np.uint32)
        k = np.asarray(key, np.uint32)
        o = np.zeros(4, np.uint32)
        self.lib.orc_philox(c.ctypes.data, k.ctypes.data, o.ctypes.data)
        return o

    def reset_counters(self):
        self.lib.orc_reset_counters()

    def counters(self):
        out = np.zeros(len(COUNTER_NAMES), np.uint64)
        self.lib.orc_get_counters(out.ctypes.data, len(COUNTER_NAMES))
        return dict(zip(COUNTER_NAMES, (int(x) for x in out)))
