"""Python face of the C++ host mirror (host/rt_host.hpp): the reference's type names
(src/*.rs `new` functions) bound through the C bindings of librt_host.so.

    host = Host()
    world = host.HittableList(); world.push(host.Sphere((0, -10, 0), 10, host.Lambertian(tex)))
    cam = host.Camera(look_from, look_at, vup, vfov, aspect, aperture, focus_dist, t0, t1)
    img = cam.render(world, nx, ny, ns)            # Camera::render — runs on the MI355X
    ppm = host.create_image(ny, nx, ns, cam, world)  # tests/test.rs:55 — P3 text

Objects are evaluated on the CPU in f64 (hit / scatter / value, like the reference) or
lowered to the flat scene of include/rtmi.h and rendered by the HIP kernels.  There is
no CPU fallback for rendering: without the extension or without a GPU, render raises.
"""
import ctypes as C
import math
import os

import numpy as np

from . import abi

PLANE_YZ, PLANE_ZX, PLANE_XY = 0, 1, 2
AXIS_X, AXIS_Y, AXIS_Z = 0, 1, 2


class HostError(RuntimeError):
    pass


class Panic(HostError):
    """Raised where the reference panics (e.g. "No bounding box in BVHNode", bvh.rs:30,58)."""


class Unsupported(HostError):
    """The object graph cannot be lowered to the device (open-ended trait impls, exotic nesting)."""


def _d3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3))


class _Obj:
    __slots__ = ("h", "keep", "host")

    def __init__(self, host, h, keep=()):
        if not h:
            host._raise()
        self.host = host
        self.h = h
        self.keep = keep


class _List(_Obj):
    def push(self, hittable):
        self.keep = self.keep + (hittable,)
        self.host._check(self.host.lib.rth_list_push(self.h, hittable.h))


def default_params(nx, ny, ns, seed=42, flags=0, max_depth=50, t_min=0.001, tile_rank=0, tile_world=1, spp_chunks=0,
                   shade_threshold=0, sample_buffer_bytes=0, progress=None):
    """progress: callable(done_units, total_units) -> falsy to go on / truthy to cancel; called from the blocking
    render calls about every 50 ms (the object returned keeps the ctypes trampoline alive as `_progress_keep`)."""
    p = abi.RenderParams()
    if progress is not None:
        def _tramp(done, total, _user):
            try:
                return 1 if progress(int(done), int(total)) else 0
            except Exception:  # nothing may unwind through the C ABI
                return 1
        cb = abi.PROGRESS_FN(_tramp)
        p._progress_keep = cb
        p.progress_fn = C.cast(cb, C.c_void_p).value
    p.nx, p.ny, p.ns = nx, ny, ns
    p.max_depth, p.t_min, p.flags, p.seed = max_depth, t_min, flags, seed
    p.tile_rank, p.tile_world, p.spp_chunks = tile_rank, tile_world, spp_chunks
    p.shade_threshold = shade_threshold
    p.sample_buffer_bytes = sample_buffer_bytes
    return p


def _coop_flags(kw, coop, flag=abi.RTMI_FLAG_LIGHT_COOP):
    """coop=True of the lighting renders: ORs RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h) into the keyword `flags`;
    the roulette renders pass their own flag, RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h)."""
    if coop:
        kw["flags"] = int(kw.get("flags", 0)) | flag
    return kw


def _batch_coop_flags(flags, coop):
    """coop=True of the batch modes: ORs RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h) into a flags word."""
    return int(flags) | (abi.FLAG_BATCH_COOP if coop else 0)


class Scene:
    """A world lowered to the flat device description (and, after upload(), resident in HBM)."""

    def __init__(self, host, world):
        self.host = host
        self.world = world
        self.h = host.lib.rth_lower(world.h)
        if not self.h:
            host._raise()
        self.uploaded = False

    def desc(self):
        d = abi.SceneDesc()
        self.host._check(self.host.lib.rth_lowered_desc(self.h, C.byref(d)))
        return d

    def arrays(self):
        """numpy views of the flat arrays (for inspection / CPU tests of the lowering)."""
        d = self.desc()

        def view(ptr, n, dtype, cols=None):
            if n == 0:
                return np.zeros((0,) if cols is None else (0, cols), dtype)
            a = np.ctypeslib.as_array(ptr, shape=(n,) if cols is None else (n, cols))
            return a.view(dtype).copy() if cols is None else a.copy()

        out = {
            "items": [d.items[i] for i in range(d.n_items)],
            "prim_a": view(d.prim_a, d.n_prims * 4, np.float32).reshape(-1, 4),
            "prim_b": view(d.prim_b, d.n_prims * 4, np.float32).reshape(-1, 4),
            "prim_meta": [d.prim_meta[i] for i in range(d.n_prims)],
            "nodes": [d.nodes[i] for i in range(d.n_nodes)],
            "xforms": [d.xforms[i] for i in range(d.n_xforms)],
            "materials": [d.materials[i] for i in range(d.n_materials)],
            "textures": [d.textures[i] for i in range(d.n_textures)],
            "n_perlin": d.n_perlin, "n_images": d.n_images, "image_bytes": d.image_bytes,
            "max_bvh_depth": d.max_bvh_depth,
            "prim_gate": view(d.prim_gate, d.n_prims * 8, np.float32).reshape(-1, 8) if d.prim_gate else np.zeros((0, 8), np.float32),
        }
        return out

    def desc_f64(self):
        """The double planes of the f64 render mode (rtmi_scene_f64, include/rtmi_f64.h)."""
        d = abi.SceneF64()
        self.host._check(self.host.lib.rth_lowered_desc_f64(self.h, C.byref(d)))
        return d

    def arrays_f64(self):
        """numpy copies of the double planes (for CPU tests of the wide lowering)."""
        d = self.desc_f64()

        def view(ptr, n, cols):
            if n == 0:
                return np.zeros((0, cols))
            return np.ctypeslib.as_array(ptr, shape=(n * cols,)).copy().reshape(n, cols)

        return {"prim_a": view(d.prim_a, d.n_prims, 4), "prim_b": view(d.prim_b, d.n_prims, 4),
                "prim_dt": view(d.prim_dt, d.n_prims, 1)[:, 0], "prim_gate": view(d.prim_gate, d.n_prims, 8),
                "nodes": view(d.nodes, d.n_nodes, 12), "xforms": view(d.xforms, d.n_xforms, 4),
                "item_neg_inv_density": view(d.item_neg_inv_density, d.n_items, 1)[:, 0],
                "item_root": view(d.item_root, d.n_items, 6), "material_param": view(d.material_param, d.n_materials, 1)[:, 0],
                "texture_f": view(d.texture_f, d.n_textures, 4), "perlin_ranvec": view(d.perlin_ranvec, d.n_perlin, 768)}

    def upload(self, device=0, f64=False, nee=False, light_tree=False):
        """Copies the scene to `device`; f64=True also attaches the double planes of the f64 render mode, nee=True the
        light table of next-event estimation (include/rtmi_nee.h), light_tree=True that table and the light tree over it
        (include/rtmi_light_tree.h; implies nee=True)."""
        self.host._check(self.host.lib.rth_upload(self.h, device))
        self.uploaded = True
        self.device = device
        self.f64_attached = False
        self.lights_attached = False
        self.light_tree_attached = False
        self.following_lights = False
        if f64:
            self.attach_f64()
        if nee or light_tree:
            self.attach_lights()
        if light_tree:
            self.attach_light_tree()
        return self

    def lights(self):
        """The light table of next-event estimation (rtmi_lights_from_desc, include/rtmi_nee.h) as a numpy structured
        array with the fields item, prim, kind, material, area, weight, select_p, cdf.  Host code: needs no GPU.  It is
        the table of the host description, desc(): after an update_prims with torch tensors that description is stale,
        as its planes are, while a handle that follows its lights (follow_lights) holds the moved table."""
        lib = abi.load_rtmi()
        d = self.desc()
        n = C.c_uint32(0)
        if lib.rtmi_lights_from_desc(C.byref(d), None, 0, C.byref(n)):
            raise HostError("rtmi_lights_from_desc: " + (lib.rtmi_last_error() or b"").decode())
        buf = (abi.Light * max(n.value, 1))()
        if lib.rtmi_lights_from_desc(C.byref(d), buf, n.value, C.byref(n)):
            raise HostError("rtmi_lights_from_desc: " + (lib.rtmi_last_error() or b"").decode())
        dt = np.dtype([("item", "<i4"), ("prim", "<i4"), ("kind", "<i4"), ("material", "<i4"), ("area", "<f8"),
                       ("weight", "<f8"), ("select_p", "<f8"), ("cdf", "<f8")])
        assert dt.itemsize == C.sizeof(abi.Light) == 48
        return np.frombuffer(bytes(buf)[:n.value * 48], dtype=dt).copy()

    def attach_lights(self):
        """Derives the light table and attaches it to the uploaded handle (rtmi_scene_attach_lights)."""
        self.host._check(self.host.lib.rth_attach_lights(self.h))
        self.lights_attached = True
        self.light_tree_attached = False  # a new table detaches the tree built over the old one
        self.following_lights = False  # ... and turns following off (follow_lights)
        return self

    def light_tree(self):
        """The light tree (rtmi_light_tree_from_desc, include/rtmi_light_tree.h) as two numpy structured arrays: nodes
        (c float32 [3], r2, power, link, pad uint32 [2]; 2 * lights of them, none for a scene without lights) and paths
        (trail, depth; one per light).  Host code: needs no GPU.  A fresh build over the host description, desc(): stale
        after an update_prims with torch tensors, and not the tree of a handle that follows its lights (follow_lights),
        which keeps the topology it was attached with (rtml_relight_desc restates it)."""
        lib = abi.load_rtmi()
        d = self.desc()
        n = C.c_uint32(0)
        if lib.rtmi_light_tree_from_desc(C.byref(d), None, 0, C.byref(n), None):
            raise HostError("rtmi_light_tree_from_desc: " + (lib.rtmi_last_error() or b"").decode())
        nodes = np.zeros(n.value, LIGHT_NODE_DTYPE)
        paths = np.zeros(n.value // 2, LIGHT_PATH_DTYPE)
        if n.value and lib.rtmi_light_tree_from_desc(C.byref(d), nodes.ctypes.data_as(C.POINTER(abi.LightNode)), n.value, C.byref(n),
                                                     paths.ctypes.data_as(C.POINTER(abi.LightPath))):
            raise HostError("rtmi_light_tree_from_desc: " + (lib.rtmi_last_error() or b"").decode())
        return nodes, paths

    def attach_light_tree(self):
        """Builds the light tree and attaches it to the uploaded handle, with the light table when that is missing
        (rtmi_scene_attach_light_tree).  A scene resident on a device list (upload_multi) raises Unsupported."""
        self.host._check(self.host.lib.rth_attach_light_tree(self.h))
        self.lights_attached = True
        self.light_tree_attached = True
        self.following_lights = False  # the tables of follow_lights index the old tree
        return self

    def _light_probe(self, op, points, aux):
        points = np.ascontiguousarray(points, dtype=np.float32)
        if points.ndim != 2 or points.shape[1] != 3 or aux.shape != (points.shape[0],):
            raise ValueError("the light tree's probes take points [n, 3] and n uniforms or light indices")
        self._ready({})
        if self.uploaded and not getattr(self, "light_tree_attached", False):
            self.attach_light_tree()
        n = points.shape[0]
        light, p = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.host._check(self.host.lib.rth_probe_light_tree(self.h, op, points.ctypes.data, aux.ctypes.data, n, light.ctypes.data,
                                                            p.ctypes.data))
        return light, p

    def light_pick(self, points, u):
        """The device's walk of the attached light tree (rtmi_probe_light_tree, PICK): for points float32 [n, 3] and
        uniforms u float32 [n] in [0, 1) the light each walk ends at (uint32 [n]) and its probability (float32 [n]).  The
        tree is attached on first use."""
        return self._light_probe(abi.RTMI_LIGHT_TREE_PROBE_PICK, points, np.ascontiguousarray(u, dtype=np.float32))

    def light_pmf(self, points, lights):
        """The device's reverse walk (rtmi_probe_light_tree, PMF): the probability (float32 [n]) that the walk from
        points[k] ends at the light lights[k] (an index into lights())."""
        return self._light_probe(abi.RTMI_LIGHT_TREE_PROBE_PMF, points, np.ascontiguousarray(lights, dtype=np.uint32))[1]

    def attach_env(self, rgb):
        """Attaches an environment map (include/rtmi_env.h): float32 [H, W, 3], row 0 the top row (+y), finite and >= 0.
        Replaces an attached map; uploads the scene first when needed."""
        a = np.asarray(rgb)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.float32:
            raise ValueError("attach_env takes a float32 [H, W, 3] array, not %s %r" % (a.dtype, a.shape))
        a = np.ascontiguousarray(a)
        if not self.uploaded:
            self.upload(0)
        self.host._check(self.host.lib.rth_attach_env(self.h, a.shape[1], a.shape[0], a.ctypes.data))
        self.env_attached = True
        return self

    def detach_env(self):
        """Frees the attached environment map (rtmi_scene_attach_env with NULL)."""
        if self.uploaded:
            self.host._check(self.host.lib.rth_attach_env(self.h, 0, 0, None))
        self.env_attached = False
        return self

    def probe_env(self, op, inp):
        """rtmi_probe_env: the device's lookup (op RTMI_ENV_PROBE_LOOKUP, inp float32 [n, 3] directions -> [n, 4] = r, g, b,
        pdf) or light sample (RTMI_ENV_PROBE_SAMPLE, inp float32 [n, 2] uniforms -> [n, 4] = direction, pdf) on the
        attached map, with p_env = 1."""
        inp = np.ascontiguousarray(inp, dtype=np.float32)
        n = inp.shape[0]
        out = np.zeros((n, 4), np.float32)
        self.host._check(self.host.lib.rth_probe_env(self.h, int(op), inp.ctypes.data, out.ctypes.data, n))
        return out

    def attach_f64(self):
        """Attaches the double planes to the uploaded handle (rtmi_scene_attach_f64)."""
        self.host._check(self.host.lib.rth_attach_f64(self.h))
        self.f64_attached = True
        return self

    def render(self, cam, nx, ny, ns, sig=False, out=None, precision="f32", **kw):
        """Blocking whole-image render -> dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], stats[, sig u64 [ny,nx]]).
        `out` = (linear, rgb8) arrays to reuse.  precision="f64": the f64 render mode (include/rtmi_f64.h) — linear is
        float64, t_min (default 0.001) is passed as a double; the double planes are attached on first use."""
        if not self.uploaded:
            self.upload(kw.pop("device", 0))
        kw.pop("device", None)
        if precision == "f64":
            return self._render_f64(cam, nx, ny, ns, sig, **kw)
        if precision != "f32":
            raise ValueError("precision must be 'f32' or 'f64'")
        p = default_params(nx, ny, ns, **kw)
        lin, rgb = out if out is not None else (np.zeros((ny, nx, 3), np.float32), np.zeros((ny, nx, 3), np.uint8))
        sg = np.zeros((ny, nx), np.uint64) if sig else None
        st = abi.Stats()
        self.host._check(self.host.lib.rth_render(self.h, cam.h, C.byref(p), lin.ctypes.data, rgb.ctypes.data,
                                                   sg.ctypes.data if sig else None, C.byref(st)))
        out = {"linear": lin, "rgb8": rgb, "stats": _stats(st)}
        if sig:
            out["sig"] = sg
        return out

    def _render_f64(self, cam, nx, ny, ns, sig, **kw):
        if not getattr(self, "f64_attached", False):
            self.attach_f64()
        t_min = float(kw.get("t_min", 0.001))
        p = default_params(nx, ny, ns, **kw)
        lin = np.zeros((ny, nx, 3), np.float64)
        rgb = np.zeros((ny, nx, 3), np.uint8)
        sg = np.zeros((ny, nx), np.uint64) if sig else None
        st = abi.Stats()
        self.host._check(self.host.lib.rth_render_f64(self.h, cam.h, C.byref(p), t_min, lin.ctypes.data, rgb.ctypes.data,
                                                       sg.ctypes.data if sig else None, C.byref(st)))
        out = {"linear": lin, "rgb8": rgb, "stats": _stats(st)}
        if sig:
            out["sig"] = sg
        return out

    def _ready(self, kw, lights=False, multi_refuses=True):
        """Before a render of the uploaded handle: uploads on first use (to the keyword `device`), drops `device` from the
        keywords and, with lights=True, attaches the light table on first use.  multi_refuses: a scene resident on a
        device list (upload_multi) is not uploaded, so that the native entry refuses it."""
        if not self.uploaded and not (multi_refuses and getattr(self, "multi_devices", None)):
            self.upload(kw.pop("device", 0))
        kw.pop("device", None)
        if lights and self.uploaded and not getattr(self, "lights_attached", False):
            self.attach_lights()

    def render_adaptive(self, cam, nx, ny, ns, min_spp, step_spp, abs_tol=0.0, rel_tol=0.0, precision="f32", nee=False,
                        env=False, env_select_p=0.5, coop=False, **kw):
        """Adaptive sampling (include/rtmi_adaptive.h): every 8x8 tile gets min_spp samples, then step_spp more per step
        while some in-image pixel has stderr > abs_tol + rel_tol * |mean|, up to ns.  Returns dict(linear f32 [ny,nx,3],
        rgb8 u8 [ny,nx,3], stderr f32 [ny,nx,3], spp u32 [ny,nx], stats).  A tile is bit for bit the tile of
        render(ns = its spp).  progress: callable(done, total) in tile-samples, total = tiles x ns.
        nee=True: the estimator of render_nee (include/rtmi_adaptive_nee.h), a tile bit for bit, stderr included, that of
        render_nee(ns = its spp); the light table is attached on first use.  env=True: that of render_env(nee=nee,
        env_select_p=env_select_p) with the attached map.  The defaults are the plain estimator.
        coop=True (with nee or env; RTMI_FLAG_LIGHT_COOP): as in render_nee; the plain estimator is cooperative by default,
        so coop=True without nee or env raises ValueError."""
        if coop and not (nee or env):
            raise ValueError("coop=True needs nee=True or env=True: the plain adaptive render is cooperative by default")
        if precision != "f32":
            raise Unsupported("adaptive sampling has no f64 mode")
        _coop_flags(kw, coop)
        self._ready(kw, lights=nee, multi_refuses=False)
        p = default_params(nx, ny, ns, **kw)
        a = abi.Adaptive(min_spp, step_spp, abs_tol, rel_tol)
        out, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr", "spp"))
        if env:
            o = abi.EnvRender(1 if nee else 0, env_select_p)
            self.host._check(self.host.lib.rth_render_adaptive_env(self.h, cam.h, C.byref(p), C.byref(o), C.byref(a), *outs))
        elif nee:
            self.host._check(self.host.lib.rth_render_adaptive_nee(self.h, cam.h, C.byref(p), C.byref(a), *outs))
        else:
            self.host._check(self.host.lib.rth_render_adaptive(self.h, cam.h, C.byref(p), C.byref(a), *outs))
        return _result(out)

    def render_features(self, cam, nx, ny, ns, sig=False, precision="f32", **kw):
        """First-hit features for denoisers (include/rtmi_features.h): the first interaction of render()'s paths, per
        sample, averaged in f64.  Returns dict(albedo f32 [ny,nx,3], normal f32 [ny,nx,3], depth f32 [ny,nx] (+inf where
        no sample hit), hits u32 [ny,nx], stats[, sig u64 [ny,nx]]); sig equals render(max_depth=0, sig=True)["sig"].
        Row 0 is the top row.  A scene resident on a device list (upload_multi) raises Unsupported."""
        if precision != "f32":
            raise Unsupported("first-hit features have no f64 mode")
        self._ready(kw)
        p = default_params(nx, ny, ns, **kw)
        out, outs = _outputs(ny, nx, ("albedo", "normal", "depth", "hits"), bool(sig))
        self.host._check(self.host.lib.rth_render_features(self.h, cam.h, C.byref(p), *outs))
        return _result(out)

    def render_nee(self, cam, nx, ny, ns, sig=False, precision="f32", coop=False, light_tree=False, **kw):
        """Next-event estimation (include/rtmi_nee.h): render()'s paths with a light sample at every diffuse vertex,
        combined by the power heuristic; an estimator of the same image.  Returns dict(linear f32 [ny,nx,3], rgb8 u8
        [ny,nx,3], stderr f32 [ny,nx,3], stats[, sig u64 [ny,nx]]); sig equals render(sig=True)["sig"].  The light table
        is attached on first use.  A scene resident on a device list (upload_multi) raises Unsupported.
        coop=True (RTMI_FLAG_LIGHT_COOP, include/rtmi_light_coop.h): under RTMI_FLAG_FAST_CULL the wave-cooperative kernel
        traces the same paths; every plane has the same bits, stats["kernel"] tells which kernel ran (scenes with
        instanced primitives or media under transforms, SYNC and renders without FAST_CULL stay per-lane).  Measured at
        64 spp on an MI355X (Timing): 1.59x faster on lit_final_scene, 1.40x on lit_random_spheres, 1.05x on
        cornell_box and 1.09x on lit_smoke (no tree to walk); it lost on no scene measured.  Opt-in all the same.
        light_tree=True (RTMI_FLAG_LIGHT_TREE, include/rtmi_light_tree.h): every vertex picks its light by walking the
        light tree from its own position instead of from the one table; same paths and sig, another estimator of the same
        image.  It pays under grids of many small lights and costs elsewhere: measured figures in DESIGN.md §25.  The tree is attached on first use.  With a
        single light the bits are those of the table's render; beside coop=True the call raises Unsupported."""
        if precision != "f32":
            raise Unsupported("next-event estimation has no f64 mode")
        _coop_flags(kw, coop)
        _coop_flags(kw, light_tree, abi.RTMI_FLAG_LIGHT_TREE)
        self._ready(kw, lights=True)
        if light_tree and self.uploaded and not getattr(self, "light_tree_attached", False):
            self.attach_light_tree()
        p = default_params(nx, ny, ns, **kw)
        out, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr"), bool(sig))
        self.host._check(self.host.lib.rth_render_nee(self.h, cam.h, C.byref(p), *outs))
        return _result(out)

    def render_env(self, cam, nx, ny, ns, nee=True, env_select_p=0.5, sig=False, precision="f32", coop=False, **kw):
        """Environment lighting (include/rtmi_env.h): render()'s paths with the attached map (attach_env) where a ray
        leaves the world; nee=True also samples the map (importance-sampled) and the area lights at every diffuse vertex,
        env_select_p being the map's share when the scene has area lights.  Returns dict(linear f32 [ny,nx,3], rgb8 u8
        [ny,nx,3], stderr f32 [ny,nx,3], stats[, sig u64 [ny,nx]]); sig equals render(sig=True)["sig"].  With nee=True the
        light table is attached on first use.  A scene resident on a device list (upload_multi) raises Unsupported.
        coop=True (RTMI_FLAG_LIGHT_COOP): as in render_nee, same bits on the wave-cooperative kernel.  Measured at 64 spp on
        an MI355X (Timing): 1.89x (nee=False) and 1.94x (nee=True) faster on random_spheres under the sun map,
        1.33x on lit_random_spheres; on earth, which has no tree, 1.04x with nee=True and level with nee=False (inside the
        spread of the repeats): the one case measured where the flag does not win.  It lost on none."""
        if precision != "f32":
            raise Unsupported("environment lighting has no f64 mode")
        _coop_flags(kw, coop)
        self._ready(kw, lights=nee)
        p = default_params(nx, ny, ns, **kw)
        o = abi.EnvRender(1 if nee else 0, env_select_p)
        out, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr"), bool(sig))
        self.host._check(self.host.lib.rth_render_env(self.h, cam.h, C.byref(p), C.byref(o), *outs))
        return _result(out)

    def _roulette_opts(self, estimator, min_depth, q_min, env_select_p, kw):
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        return abi.Roulette(abi.ROULETTE_ESTIMATORS[estimator], min_depth, q_min, env_select_p)

    def render_roulette(self, cam, nx, ny, ns, estimator="nee", min_depth=3, q_min=0.05, env_select_p=0.5, precision="f32",
                        coop=False, **kw):
        """Russian-roulette path termination (include/rtmi_roulette.h): the paths of render(), each ended after a scatter
        at depth >= min_depth with probability 1 - q, q = clamp(largest channel of the throughput, q_min, 1), the
        survivors weighted 1 / q.  estimator: "plain" (render), "nee" (render_nee), "env" (render_env(nee=False)) or
        "env_nee" (render_env(nee=True, env_select_p)).  Returns dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], stderr f32
        [ny,nx,3], bounces u32 [ny,nx] = the scatters of the pixel's paths, summed, stats).  min_depth > max_depth or
        q_min = 1 gives the named render bit for bit.
        coop=True (RTMI_FLAG_ROULETTE_COOP, include/rtmi_roulette_coop.h): under RTMI_FLAG_FAST_CULL the wave-cooperative
        kernel traces the same paths; every plane, bounces included, has the same bits, stats["kernel"] tells which kernel
        ran (scenes with instanced primitives or media under transforms, SYNC and renders without FAST_CULL stay
        per-lane).  Timing: DESIGN.md §20."""
        if precision != "f32":
            raise Unsupported("Russian roulette has no f64 mode")
        _coop_flags(kw, coop, abi.RTMI_FLAG_ROULETTE_COOP)
        o = self._roulette_opts(estimator, min_depth, q_min, env_select_p, kw)
        p = default_params(nx, ny, ns, **kw)
        out, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr", "bounces"))
        self.host._check(self.host.lib.rth_render_roulette(self.h, cam.h, C.byref(p), C.byref(o), *outs))
        return _result(out)

    def render_adaptive_roulette(self, cam, nx, ny, ns, min_spp, step_spp, abs_tol=0.0, rel_tol=0.0, estimator="nee",
                                 min_depth=3, q_min=0.05, env_select_p=0.5, precision="f32", coop=False,
                                 **kw):
        """render_roulette under the noise target of render_adaptive (ns is the cap).  Returns render_roulette's dict plus
        spp u32 [ny,nx]; a tile that stops at n samples is bit for bit, bounces included, that tile of
        render_roulette(ns=n).  coop=True (RTMI_FLAG_ROULETTE_COOP): as in render_roulette, same bits, spp included, on the
        wave-cooperative kernel."""
        if precision != "f32":
            raise Unsupported("Russian roulette has no f64 mode")
        _coop_flags(kw, coop, abi.RTMI_FLAG_ROULETTE_COOP)
        o = self._roulette_opts(estimator, min_depth, q_min, env_select_p, kw)
        p = default_params(nx, ny, ns, **kw)
        a = abi.Adaptive(min_spp, step_spp, abs_tol, rel_tol)
        out, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr", "spp", "bounces"))
        self.host._check(self.host.lib.rth_render_adaptive_roulette(self.h, cam.h, C.byref(p), C.byref(o), C.byref(a), *outs))
        return _result(out)

    def session(self, cam, nx, ny, estimator="plain", roulette=None, env_select_p=0.5, first_sample=0, lattice=None, coop=False,
                **kw):
        """A render session (include/rtmi_session.h): the accumulation state of a render kept across calls, so that it can
        be continued, refined, read at any point, saved, restored and merged.  estimator: "plain", "nee", "env" or
        "env_nee"; roulette: None or dict(min_depth, q_min) (rtmi_roulette.h); first_sample: the session's samples are
        [first_sample, first_sample + n); lattice: None for a FIXED session (Session.render) or (min_spp, step_spp) for a
        REFINE session (Session.refine).  coop=True selects the wave-cooperative kernel under the rule of the estimator's
        one-shot entry.  The other keywords are default_params' (ns is not read).  The light table is attached on first use.
        A scene resident on a device list (upload_multi) raises Unsupported."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        rr = roulette is not None
        _coop_flags(kw, coop, abi.RTMI_FLAG_ROULETTE_COOP if rr else abi.RTMI_FLAG_LIGHT_COOP)
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        p = default_params(nx, ny, 1, **kw)
        min_spp, step_spp = (0, 0) if lattice is None else lattice
        o = abi.SessionOpts(abi.ROULETTE_ESTIMATORS[estimator], 1 if rr else 0, roulette["min_depth"] if rr else 0,
                            roulette["q_min"] if rr else 0.0, env_select_p, first_sample, min_spp, step_spp)
        h = self.host.lib.rth_session_create(self.h, cam.h, C.byref(p), C.byref(o))
        if not h:
            self.host._raise()
        return Session(self.host, h, nx, ny, keep=(self, cam, p))

    def render_denoised(self, cam, nx, ny, ns, denoise=None, nee=False, env=False, coop=False, **kw):
        """A render and its denoised image: render_adaptive(min_spp=ns, step_spp=1) (render()'s image plus its standard
        errors), render_features with the same ns and keywords, then denoise() of the three on the scene's device.
        `denoise` = dict of denoise() keywords.  Returns dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], noisy = the adaptive
        dict, features = the features dict).  ns >= 2; the other restrictions are those of the two renders.
        nee=True: the noisy image and its standard errors come from render_nee (the same paths, so the features still
        describe them).  env=True: they come from render_env(nee=nee) with the attached map (env_select_p among the
        keywords); pixels where no sample hits a surface are not filtered: they keep the map as seen.
        coop=True (with nee or env): the lit render gets RTMI_FLAG_LIGHT_COOP (render_nee); render_features does not."""
        if ns < 2:
            raise ValueError("render_denoised needs ns >= 2 (a standard error needs two samples)")
        if coop and not (nee or env):
            raise ValueError("coop=True needs nee=True or env=True: the plain adaptive render is cooperative by default")
        if env:
            noisy = self.render_env(cam, nx, ny, ns, nee=nee, coop=coop, **kw)
            kw.pop("env_select_p", None)
        elif nee:
            noisy = self.render_nee(cam, nx, ny, ns, coop=coop, **kw)
        else:
            noisy = self.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, **kw)
        kw.pop("device", None)
        ft = self.render_features(cam, nx, ny, ns, **kw)
        out = _denoise(noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"],
                       device=self.device, **(denoise or {}))
        return {"linear": out["linear"], "rgb8": out["rgb8"], "noisy": noisy, "features": ft}

    def render_temporal(self, temporal, cam, nx, ny, ns, denoise=None, nee=False, env=False, coop=False, **kw):
        """One frame of a sequence: render_denoised's two renders, then temporal.push (a Temporal of this size) of the
        noisy image, its standard errors and the features under `cam`, then denoise() of the pushed linear and stderr
        with this frame's features.  Returns render_denoised's dict plus accumulated = the push's dict.  denoise=False
        skips the filter: linear is the accumulated image and rgb8 its quantisation (denoise() with iterations=0)."""
        if ns < 2:
            raise ValueError("render_temporal needs ns >= 2 (a standard error needs two samples)")
        if coop and not (nee or env):
            raise ValueError("coop=True needs nee=True or env=True: the plain adaptive render is cooperative by default")
        if env:
            noisy = self.render_env(cam, nx, ny, ns, nee=nee, coop=coop, **kw)
            kw.pop("env_select_p", None)
        elif nee:
            noisy = self.render_nee(cam, nx, ny, ns, coop=coop, **kw)
        else:
            noisy = self.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, **kw)
        kw.pop("device", None)
        ft = self.render_features(cam, nx, ny, ns, **kw)
        acc = temporal.push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"])
        opts = {"iterations": 0} if denoise is False else (denoise or {})
        out = _denoise(acc["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=acc["stderr"], device=self.device, **opts)
        return {"linear": out["linear"], "rgb8": out["rgb8"], "noisy": noisy, "features": ft, "accumulated": acc}

    def frame(self, nx, ny, estimator="plain", temporal=(), denoise=(), coop=False, env_select_p=0.5, **kw):
        """A frame handle (include/rtmi_frame.h): render_temporal's chain of five calls as one, with every plane kept on
        the device between the stages and all device memory allocated here, once.  estimator: "plain",
        "nee", "env" or "env_nee" (render_temporal's nee and env); temporal: dict of Temporal's keywords ({} or omitted: its
        defaults) or None for no history (render_denoised's chain); denoise: dict of denoise()'s keywords ({} or omitted:
        its defaults) or False for no filter (render_temporal(denoise=False)); coop=True (with a lit estimator): the lit
        render gets RTMI_FLAG_LIGHT_COOP.  The other keywords are default_params' (ns and seed are Frame.render's).  The
        light table is attached on first use.  A scene resident on a device list (upload_multi) raises Unsupported."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        if coop and estimator == "plain":
            raise ValueError("coop=True needs a lit estimator: the plain render is cooperative by default")
        _coop_flags(kw, coop)
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        p = default_params(nx, ny, 2, **kw)
        o = abi.FrameOpts(abi.ROULETTE_ESTIMATORS[estimator], env_select_p, _temporal_params(**dict(temporal or ())),
                          _denoise_params(**dict(denoise or ())),
                          (abi.RTMI_FRAME_NO_TEMPORAL if temporal is None else 0) | (abi.RTMI_FRAME_NO_FILTER if denoise is False else 0))
        h = self.host.lib.rth_frame_create(self.h, C.byref(p), C.byref(o))
        if not h:
            self.host._raise()
        return Frame(self.host, h, nx, ny, self.device, temporal is not None, keep=(self, p))

    def upscaler(self, nx, ny, low=None, scale=2.0, guide_ns=4, estimator="plain", temporal=(), denoise=(), coop=False,
                 env_select_p=0.5, upscale=None, **kw):
        """An upscaler handle (include/rtmi_upscale.h): a frame handle at a low resolution whose image is
        rebuilt at nx x ny on the device, guided by first-hit features rendered at the full size with guide_ns samples per
        pixel.  low = (lx, ly): the low resolution; otherwise scale gives lx = ceil(nx / scale), ly = ceil(ny / scale).
        estimator, temporal, denoise, coop, env_select_p and the other keywords: Scene.frame's, for the low frame.
        upscale: dict of upscale()'s parameter keywords ({} or None: its defaults).  All device memory is allocated here,
        once.  A scene resident on a device list (upload_multi) raises Unsupported."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        if coop and estimator == "plain":
            raise ValueError("coop=True needs a lit estimator: the plain render is cooperative by default")
        if low is None:
            if not scale >= 1.0:
                raise ValueError("scale must be at least 1")
            low = (int(math.ceil(nx / scale)), int(math.ceil(ny / scale)))
        lx, ly = int(low[0]), int(low[1])
        _coop_flags(kw, coop)
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        p = default_params(nx, ny, 2, **kw)
        fo = abi.FrameOpts(abi.ROULETTE_ESTIMATORS[estimator], env_select_p, _temporal_params(**dict(temporal or ())),
                           _denoise_params(**dict(denoise or ())),
                           (abi.RTMI_FRAME_NO_TEMPORAL if temporal is None else 0) | (abi.RTMI_FRAME_NO_FILTER if denoise is False else 0))
        o = abi.UpscalerOpts(fo, _upscale_params(**dict(upscale or ())), lx, ly, guide_ns)
        h = self.host.lib.rth_upscaler_create(self.h, C.byref(p), C.byref(o))
        if not h:
            self.host._raise()
        return Upscaler(self.host, h, nx, ny, lx, ly, self.device, keep=(self, p))

    def render_multi(self, cam, nx, ny, ns, devices, **kw):
        """Whole image on several GPUs of this process (rtmi_render_multi): tiles t % len(devices), one gather.
        A device may be listed more than once (single-GPU rehearsal).  Bit-identical to render()."""
        p = default_params(nx, ny, ns, **kw)
        lin = np.zeros((ny, nx, 3), np.float32)
        rgb = np.zeros((ny, nx, 3), np.uint8)
        st = abi.Stats()
        dev = (C.c_int * len(devices))(*devices)
        self.host._check(self.host.lib.rth_render_multi(self.h, cam.h, C.byref(p), dev, len(devices), lin.ctypes.data,
                                                         rgb.ctypes.data, C.byref(st)))
        return {"linear": lin, "rgb8": rgb, "stats": _stats(st)}

    def partial_image(self, nx, ny, ns):
        """RTMI_FLAG_PROGRESSIVE: the image of the passes finished so far of the render() call running on this scene —
        ONLY from inside that call's progress callback.  Returns (spp_done, linear, rgb8); spp_done == 0: nothing yet."""
        p = default_params(nx, ny, ns)
        lin = np.zeros((ny, nx, 3), np.float32)
        rgb = np.zeros((ny, nx, 3), np.uint8)
        spp = C.c_uint32(0)
        self.host._check(self.host.lib.rth_partial_image(self.h, C.byref(p), lin.ctypes.data, rgb.ctypes.data, C.byref(spp)))
        return int(spp.value), lin, rgb

    def upload_multi(self, devices):
        """Keeps the scene resident on a list of GPUs of this process (rtmi_multi_create): uploads once; every later
        render_resident() costs the kernels, one gather and the un-tiling.  A device may be listed more than once."""
        dev = (C.c_int * len(devices))(*devices)
        self.host._check(self.host.lib.rth_upload_multi(self.h, dev, len(devices)))
        self.multi_devices = list(devices)
        return self

    def multi_collective(self):
        """Which exchange render_resident() performs: "none" (one device), "peer_copy" (a device listed twice) or
        "rccl" (one grouped ncclGather; distinct devices, or one device with RTMI_FORCE_RCCL=1 at upload_multi)."""
        return {0: "none", 1: "peer_copy", 2: "rccl"}.get(self.host.lib.rth_multi_collective(self.h), "no handle")

    def free_multi(self):
        self.host._check(self.host.lib.rth_multi_free(self.h))
        self.multi_devices = None
        return self

    def prepare_resident(self, nx, ny, ns, **kw):
        p = default_params(nx, ny, ns, **kw)
        self.host._check(self.host.lib.rth_multi_prepare(self.h, C.byref(p)))
        return self

    def render_resident(self, cam, nx, ny, ns, out=None, **kw):
        """rtmi_multi_render on the device list of upload_multi().  `out` = (linear, rgb8) arrays to reuse."""
        p = default_params(nx, ny, ns, **kw)
        lin, rgb = out if out is not None else (np.zeros((ny, nx, 3), np.float32), np.zeros((ny, nx, 3), np.uint8))
        st = abi.Stats()
        self.host._check(self.host.lib.rth_multi_render(self.h, cam.h, C.byref(p), lin.ctypes.data, rgb.ctypes.data, C.byref(st)))
        return {"linear": lin, "rgb8": rgb, "stats": _stats(st)}

    def check_status(self):
        """Raises if an asynchronous render_device() call since the last check overflowed its traversal pool."""
        self.host._check(self.host.lib.rth_scene_status(self.h))
        return self

    def local_tiles(self, params):
        return abi.load_rtmi().rtmi_local_tiles(C.byref(params))

    def prepare(self, params):
        """Allocate the render buffers for `params` now (per-sample buffer: 12 B x local pixels x samples per pass)."""
        self.host._check(self.host.lib.rth_render_prepare(self.h, C.byref(params)))
        return self

    def render_device(self, cam, params, d_texels_ptr, stream=None, want_stats=False):
        """Enqueue on `stream`; writes rtmi_local_tiles()*64 texels (16 B) at device address d_texels_ptr."""
        st = abi.Stats() if want_stats else None
        self.host._check(self.host.lib.rth_render_device(self.h, cam.h, C.byref(params), C.c_void_p(d_texels_ptr),
                                                          C.c_void_p(stream or 0), C.byref(st) if st else None))
        return _stats(st) if st else None

    # ---- scene updates (include/rtmi_update.h): edits of the FLAT scene.  The host object graph this scene was lowered from
    # (host.hit(...), a new host.lower(world)) keeps the old positions, and so do the double planes of the f64 mode.
    def refittable(self):
        """Per item of the description whether update_prims can refit it (rtmu_refittable): bool [n_items], True for the BVH
        items whose primitives may move; LIST items are False, their primitives sit under no box and may always move."""
        mask = np.zeros(max(self.desc().n_items, 1), np.uint8)
        self.host._check(self.host.lib.rthu_refittable(self.h, mask.ctypes.data))
        return mask[:self.desc().n_items] != 0

    def _emitters_in(self, first, count):
        """whether the range holds a primitive with a DIFFUSE_LIGHT material: a slice of a mask computed once (types and
        materials do not change under the updates)"""
        if getattr(self, "_emits", None) is None:
            d = self.desc()
            meta = np.ctypeslib.as_array(C.cast(d.prim_meta, C.POINTER(C.c_int32)), shape=(d.n_prims, 4)) if d.n_prims else np.zeros((0, 4), np.int32)
            kinds = np.ctypeslib.as_array(C.cast(d.materials, C.POINTER(C.c_int32)), shape=(d.n_materials, 4))[:, 0] if d.n_materials else np.zeros(0, np.int32)
            self._emits = kinds[meta[:, 0]] == abi.MAT_DIFFUSE_LIGHT  # (a copy: fancy indexing)
        return bool(self._emits[first:first + count].any())

    def follow_lights(self, on=True):
        """The attached light table and light tree follow the updates of this handle (rtml_scene_follow_lights,
        include/rtmi_relight.h): an update_prims whose range holds an emitter then recomputes the table and refits the tree
        on the device, behind the refit of the BVH items, instead of detaching them — in both forms, so torch tensors may
        move the lamps.  Needs an uploaded scene with the light table attached (the tree too, if it is to follow); builds
        the handle's tables now, waiting for the calls enqueued on it.  The tree keeps the topology it was attached with.
        upload(), attach_lights() and attach_light_tree() turn following off again; on=False does so explicitly."""
        self.host._check(self.host.lib.rthl_follow_lights(self.h, 1 if on else 0))
        self.following_lights = bool(on)
        return self

    def light_words(self, which):
        """One of the resident handle's light arrays as bytes (rtml_probe_light_words, a test hook): `which` is a key of
        abi.LIGHT_WORDS.  Waits for the calls enqueued on the handle."""
        need = C.c_size_t(0)
        self.host._check(self.host.lib.rthl_probe_light_words(self.h, abi.LIGHT_WORDS[which], None, 0, C.byref(need)))
        out = np.zeros(need.value, np.uint8)
        if need.value:
            self.host._check(self.host.lib.rthl_probe_light_words(self.h, abi.LIGHT_WORDS[which], out.ctypes.data, need.value, None))
        return out

    def prepare_updates(self):
        """Builds the resident handle's update tables now (rtmu_scene_update_prepare): otherwise its first update does,
        waiting for the calls enqueued on the handle and allocating — also the first update with torch tensors."""
        self.host._check(self.host.lib.rthu_update_prepare(self.h))
        return self

    def update_prims(self, first, a, b=None):
        """New planes A (and B) for the primitives [first, first + len(a)) of the scene, resident or not; a, b: float32
        [n, 4] (rtmi.h, "primitives"); b=None keeps the planes B.  The trees of every BVH item the range touches are refit
        on the device (rtmu_scene_update_prims); every handle bound to the scene stays valid.

        numpy arrays: blocking.  The planes are also written into the lowered arrays and refit there (rtmu_refit_desc), so
        desc() stays the description of what is resident; when the range holds an emitter, the light table and the light
        tree that were attached are derived again from it and re-attached — unless the handle follows its lights
        (follow_lights): then the device recomputes both behind the refit and nothing is re-attached.

        torch tensors on the scene's device: asynchronous on the current stream, no host copy (the _device entry) — and
        the lowered arrays go STALE: desc(), arrays() and everything derived from them describe the scene before the
        update.  Raises when the range holds an emitter while a light table is attached, which would have to be derived
        from the stale description — unless the handle follows its lights (follow_lights): then the update also recomputes
        the table and refits the light tree on the device, still without a wait or an allocation.  Inside refittable items finite planes, non-zero radii and cubes with min <= max are
        the caller's contract.  The handle's first update waits for the handle and allocates: see prepare_updates().

        Either form leaves the double planes of the f64 render mode at the positions the scene was lowered with: after an
        update attach_f64() and render(precision="f64") raise Unsupported (and with the planes attached the update does)."""
        if type(a).__module__.split(".")[0] == "torch":
            return self._update_prims_torch(first, a, b)
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 4 or (b is not None and b.shape != a.shape):
            raise ValueError("update_prims takes float32 [n, 4] planes")
        first, n = int(first), a.shape[0]
        if first < 0 or first + n > self.desc().n_prims:
            raise ValueError("primitives [%d, %d) are outside the scene's %d" % (first, first + n, self.desc().n_prims))
        relight = (n > 0 and self.uploaded and getattr(self, "lights_attached", False) and not getattr(self, "following_lights", False)
                   and self._emitters_in(first, n))
        tree = relight and getattr(self, "light_tree_attached", False)
        self.host._check(self.host.lib.rthu_update_prims(self.h, first, n, a.ctypes.data, b.ctypes.data if b is not None else None))
        if relight:
            self.lights_attached = self.light_tree_attached = False
            self.attach_lights()
            if tree:
                self.attach_light_tree()
        return self

    def _update_prims_torch(self, first, a, b):
        import torch

        if not self.uploaded:
            raise HostError("update_prims with tensors needs an uploaded scene")
        for t in (a,) if b is None else (a, b):
            dev = t.device
            if dev.type != "cuda" or (dev.index or 0) != self.device:
                raise ValueError("the planes are on %s, the scene is on device %d" % (dev, self.device))
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 4 or t.shape != a.shape or not t.is_contiguous():
                raise ValueError("update_prims takes contiguous float32 [n, 4] planes")
        first, n = int(first), a.shape[0]
        if first < 0 or first + n > self.desc().n_prims:
            raise ValueError("primitives [%d, %d) are outside the scene's %d" % (first, first + n, self.desc().n_prims))
        if n and getattr(self, "lights_attached", False) and not getattr(self, "following_lights", False) and self._emitters_in(first, n):
            raise HostError("update_prims with tensors: the range holds an emitter and a light table is attached; the table "
                            "would have to be derived from the stale host description (use numpy planes, or follow_lights())")
        self.host._check(self.host.lib.rthu_update_prims_device(
            self.h, first, n, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()) if b is not None else None,
            C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)))
        return self

    def update_xforms(self, first, records):
        """Replaces the transform records [first, first + len(records)) of the flat scene (rtmu_scene_update_xforms):
        records of the chains of top-level items (Traslate / Rotate around an item) and of list primitives' own chains.
        records: abi.Xform objects or (kind, x, y, z) tuples — TRANSLATE: the offset; ROTATE_*: x = sin, y = cos of the
        angle, as the lowering writes them; every record keeps its kind.  Blocking; the lowered array follows, so desc()
        stays the description of what is resident.  No tree changes: items sit in a list, not under a box."""
        recs = (abi.Xform * max(len(records), 1))(*[r if isinstance(r, abi.Xform) else abi.Xform(int(r[0]), r[1], r[2], r[3])
                                                    for r in records])
        self.host._check(self.host.lib.rthu_update_xforms(self.h, int(first), len(records), recs))
        return self

    def prims_of(self, obj):
        """The indices (uint32, ascending) of the primitives of the flat scene that were lowered from a host object: from a
        primitive itself, or from everything below a wrapper, a list, a ConstantMedium or a BVHNode."""
        n = C.c_uint32(0)
        self.host._check(self.host.lib.rthu_prims_of(self.h, obj.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            self.host._check(self.host.lib.rthu_prims_of(self.h, obj.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def device_words(self, which):
        """One of the resident handle's device arrays as bytes (rtmu_probe_scene_words, a test hook): `which` is a key of
        abi.SCENE_WORDS.  Waits for the calls enqueued on the handle."""
        need = C.c_size_t(0)
        self.host._check(self.host.lib.rthu_probe_scene_words(self.h, abi.SCENE_WORDS[which], None, 0, C.byref(need)))
        out = np.zeros(need.value, np.uint8)
        if need.value:
            self.host._check(self.host.lib.rthu_probe_scene_words(self.h, abi.SCENE_WORDS[which], out.ctypes.data, need.value, None))
        return out

    def trace(self, origins, directions, times=None, t_min=0.001, t_max=float("inf"), seed=0, first_ray=0,
              flags=abi.RTMI_FLAG_FAST_CULL):
        """Closest hits of a batch of rays (include/rtmi_query.h): for ray i the record of the reference's
        world.hit(Ray(origins[i], directions[i], times[i]), t_min, t_max), with ConstantMedium draws from the Philox stream
        keyed seed + first_ray + i.  origins, directions: float32 [n, 3]; times: [n] or None (time 0); t_min, t_max: a
        scalar or [n] each (t_max = inf: the render's).  Returns dict(hit bool [n], t, u, v [n], p, normal [n, 3], item,
        prim, material int32 [n]); a miss has t = +inf, the indices -1 and the rest 0.  flags: RTMI_FLAG_FAST_CULL or 0
        (the reference-topology traversal), same results.  A ray that starts in the plane of a rect or a cube face
        with that component of the direction +-0 (or so small that its reciprocal overflows) is accepted there with t = NaN, as in the reference (t, u, v, p are NaN); below a BVH the leaf
        that is returned for such a ray can differ from the reference's (include/rtmi_query.h, in-plane rays).
        With torch tensors on the scene's device the call is enqueued on torch's current stream (rtmi_trace_device) and
        returns torch tensors on that device: no host copy is made.  A scene resident on a device list raises Unsupported."""
        return self._query(False, origins, directions, times, t_min, t_max, seed, first_ray, flags)

    def occluded(self, origins, directions, times=None, t_min=0.001, t_max=float("inf"), seed=0, first_ray=0,
                 flags=abi.RTMI_FLAG_FAST_CULL):
        """bool [n]: whether trace() of the same arguments finds a hit — the same predicate with the same draws, by a
        scan that stops at the first accepted hit (rtmi_occluded, include/rtmi_query.h).  An in-plane ray that a rect
        accepts with t = NaN is occluded, as trace() reports it hit."""
        return self._query(True, origins, directions, times, t_min, t_max, seed, first_ray, flags)

    def _query(self, any_hit, origins, directions, times, t_min, t_max, seed, first_ray, flags):
        self._ready({})
        lib = self.host.lib
        if hasattr(origins, "data_ptr") and hasattr(origins, "is_cuda"):
            return self._query_torch(any_hit, origins, directions, times, t_min, t_max, seed, first_ray, flags)
        o, d = (np.ascontiguousarray(a, dtype=np.float32) for a in (origins, directions))
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and directions are [n, 3] arrays, not %r and %r" % (o.shape, d.shape))
        n = o.shape[0]
        rays = np.empty(n, RAY_DTYPE)
        rays["o"], rays["d"], rays["t_min"], rays["t_max"] = o, d, t_min, t_max
        tm = None if times is None else np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float32), (n,)))
        p = abi.QueryParams(n, int(flags), int(seed) & (2 ** 64 - 1), int(first_ray) & (2 ** 64 - 1))
        ms = C.c_double(0.0)
        out = np.zeros(n, np.uint8 if any_hit else HIT_DTYPE)
        fn = lib.rth_occluded if any_hit else lib.rth_trace
        self.host._check(fn(self.h, C.byref(p), rays.ctypes.data, None if tm is None else tm.ctypes.data, out.ctypes.data,
                            C.byref(ms)))
        if any_hit:
            return out.astype(bool)
        res = {k: np.ascontiguousarray(out[k]) for k in ("t", "u", "v", "p", "item", "prim", "material")}
        res["normal"] = np.ascontiguousarray(out["n"])
        res["hit"] = res["item"] >= 0
        res["kernel_ms"] = ms.value
        return res

    def _query_torch(self, any_hit, origins, directions, times, t_min, t_max, seed, first_ray, flags):
        import torch

        dev = origins.device
        if dev.type != "cuda" or (dev.index or 0) != self.device:
            raise ValueError("the rays are on %s, the scene is on device %d" % (dev, self.device))
        if origins.dtype != torch.float32 or directions.dtype != torch.float32 or origins.dim() != 2 or \
                origins.shape[1] != 3 or directions.shape != origins.shape or directions.device != dev:
            raise ValueError("origins and directions are float32 [n, 3] tensors on one device")
        n = origins.shape[0]
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        rays[:, 0:3], rays[:, 4:7] = origins, directions
        rays[:, 3] = torch.as_tensor(t_min, dtype=torch.float32, device=dev)
        rays[:, 7] = torch.as_tensor(t_max, dtype=torch.float32, device=dev)
        tm = None if times is None else torch.as_tensor(times, dtype=torch.float32, device=dev).expand(n).contiguous()
        out = torch.empty((n,), dtype=torch.uint8, device=dev) if any_hit else torch.empty((n, 12), dtype=torch.float32, device=dev)
        if n:
            p = abi.QueryParams(n, int(flags), int(seed) & (2 ** 64 - 1), int(first_ray) & (2 ** 64 - 1))
            fn = self.host.lib.rth_occluded_device if any_hit else self.host.lib.rth_trace_device
            self.host._check(fn(self.h, C.byref(p), C.c_void_p(rays.data_ptr()), C.c_void_p(tm.data_ptr()) if tm is not None else None,
                                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if any_hit:
            return out != 0
        ids = out[:, 9:12].contiguous().view(torch.int32)
        return {"hit": ids[:, 0] >= 0, "t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "p": out[:, 3:6], "normal": out[:, 6:9],
                "item": ids[:, 0], "prim": ids[:, 1], "material": ids[:, 2]}

    def radiance(self, origins, directions, times=None, spp=1, estimator="plain", t_min=0.001, t_max=float("inf"), seed=0,
                 first_ray=0, first_sample=0, stream_skip=0, max_depth=50, env_select_p=0.5, flags=abi.RTMI_FLAG_FAST_CULL,
                 samples=False, path_t_min=0.001, coop=False):
        """Path-traced radiance along a batch of rays (include/rtmi_radiance.h): spp independent paths of render()'s
        integrator per ray, each starting with the caller's ray instead of a camera ray.  estimator: "plain" (render),
        "nee" (render_nee), "env" (render_env(nee=False)) or "env_nee" (render_env(nee=True, env_select_p)); the light
        table is attached on first use, the map is the one of attach_env.  origins, directions: float32 [n, 3]; times: [n]
        or None (time 0); t_min, t_max: a scalar or [n] each, the interval of the FIRST segment (t_max = inf: the
        render's); path_t_min: the t_min of every later segment and of shadow rays.  Path (i, s) is the render's path of
        pixel index first_ray + i, sample first_sample + s under `seed`, its stream read from word stream_skip on: with
        stream_skip = 3 the rays and times of a pinhole camera give that render's samples bit for bit.
        Returns dict(mean f32 [n, 3], stderr f32 [n, 3] (+inf for spp = 1), kernel_ms[, samples f32 [n, spp, 3]]).
        With torch tensors on the scene's device the call is enqueued on torch's current stream (rtmi_radiance_device) and
        returns torch tensors on that device (samples always among them: the buffer is the kernel's): no host copy is
        made.  A scene resident on a device list raises Unsupported.
        coop=True (RTMI_FLAG_BATCH_COOP, include/rtmi_batch_coop.h): under RTMI_FLAG_FAST_CULL the wave-cooperative kernel
        traces the paths where the scene allows it, the same bits in every output.  The dict does not change: these entries
        have no rtmi_stats to report the kernel in."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        self._ready({}, lights=estimator in ("nee", "env_nee"))
        torch_in = hasattr(origins, "data_ptr") and hasattr(origins, "is_cuda")
        n = int(origins.shape[0])
        flags = _batch_coop_flags(flags, coop)
        p = abi.RadianceParams(n, int(spp), abi.ROULETTE_ESTIMATORS[estimator], int(flags), int(max_depth), float(path_t_min),
                               int(seed) & (2 ** 64 - 1), int(first_ray) & (2 ** 64 - 1), int(first_sample), int(stream_skip),
                               float(env_select_p))
        if torch_in:
            return self._radiance_torch(p, origins, directions, times, t_min, t_max)
        o, d = (np.ascontiguousarray(a, dtype=np.float32) for a in (origins, directions))
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and directions are [n, 3] arrays, not %r and %r" % (o.shape, d.shape))
        rays = np.empty(n, RAY_DTYPE)
        rays["o"], rays["d"], rays["t_min"], rays["t_max"] = o, d, t_min, t_max
        tm = None if times is None else np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float32), (n,)))
        ms = C.c_double(0.0)
        res = {"mean": np.zeros((n, 3), np.float32), "stderr": np.zeros((n, 3), np.float32)}
        if samples:
            res["samples"] = np.zeros((n, max(int(spp), 0), 3), np.float32)
        self.host._check(self.host.lib.rth_radiance(self.h, C.byref(p), rays.ctypes.data, None if tm is None else tm.ctypes.data,
                                                     res["mean"].ctypes.data, res["stderr"].ctypes.data,
                                                     res["samples"].ctypes.data if samples else None, C.byref(ms)))
        res["kernel_ms"] = ms.value
        return res

    def _radiance_torch(self, p, origins, directions, times, t_min, t_max):
        import torch

        dev = origins.device
        if dev.type != "cuda" or (dev.index or 0) != self.device:
            raise ValueError("the rays are on %s, the scene is on device %d" % (dev, self.device))
        if origins.dtype != torch.float32 or directions.dtype != torch.float32 or origins.dim() != 2 or \
                origins.shape[1] != 3 or directions.shape != origins.shape or directions.device != dev:
            raise ValueError("origins and directions are float32 [n, 3] tensors on one device")
        n = p.n
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        rays[:, 0:3], rays[:, 4:7] = origins, directions
        rays[:, 3] = torch.as_tensor(t_min, dtype=torch.float32, device=dev)
        rays[:, 7] = torch.as_tensor(t_max, dtype=torch.float32, device=dev)
        tm = None if times is None else torch.as_tensor(times, dtype=torch.float32, device=dev).expand(n).contiguous()
        res = {"mean": torch.empty((n, 3), dtype=torch.float32, device=dev), "stderr": torch.empty((n, 3), dtype=torch.float32, device=dev),
               "samples": torch.empty((n, p.spp, 3), dtype=torch.float32, device=dev)}
        # every check of the entry is made for an empty batch too; it then launches nothing
        self.host._check(self.host.lib.rth_radiance_device(
            self.h, C.byref(p), C.c_void_p(rays.data_ptr()), C.c_void_p(tm.data_ptr()) if tm is not None else None,
            C.c_void_p(res["mean"].data_ptr()), C.c_void_p(res["stderr"].data_ptr()), C.c_void_p(res["samples"].data_ptr()),
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return res

    def irradiance(self, points, normals, spp, seed=0, coop=False, **kw):
        """Irradiance at surface points (probes, lightmap and vertex baking): E = integral of L cos(theta) over the
        normal's hemisphere, estimated with spp cosine-distributed directions per point (irradiance_directions, drawn on
        the host from Philox under `seed`), one radiance() path along each: E = pi * mean.  points, normals: [n, 3];
        normals need not be unit length.  kw: radiance()'s keywords (estimator, max_depth, t_min, flags, ...); the rays are
        stream_skip = 0 rays starting at the point, ray k of point i being ray i * spp + k of the batch.
        Returns dict(irradiance f32 [n, 3], stderr f32 [n, 3]): the standard error of the estimate from the per-ray
        values (+inf for spp = 1).  coop=True: radiance()'s."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3 or nrm.shape != pts.shape:
            raise ValueError("points and normals are [n, 3] arrays, not %r and %r" % (pts.shape, nrm.shape))
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be at least 1")
        for k in ("spp", "samples", "stream_skip", "times"):
            if k in kw:
                raise ValueError("irradiance() sets %s itself" % k)
        n = pts.shape[0]
        dirs = irradiance_directions(nrm, spp, seed)
        r = self.radiance(np.repeat(pts, spp, axis=0), dirs.reshape(n * spp, 3), spp=1, seed=seed, stream_skip=0, coop=coop, **kw)
        x = r["mean"].astype(np.float64).reshape(n, spp, 3)
        mean = x.sum(axis=1) / float(spp)
        if spp > 1:
            se = np.sqrt(((x - mean[:, None, :]) ** 2).sum(axis=1) / (float(spp) * (float(spp) - 1.0)))
        else:
            se = np.full((n, 3), np.inf)
        return {"irradiance": (np.pi * mean).astype(np.float32), "stderr": (np.pi * se).astype(np.float32)}

    def gather(self, points, normals=None, spp=16, mode="cosine", estimator="plain", seed=0, first_point=0, first_sample=0,
               slab_points=0, times=None, flags=abi.RTMI_FLAG_FAST_CULL, max_depth=50, t_min=0.001, env_select_p=0.5, sh=True,
               scratch_bytes=None, coop=False):
        """Light arriving at points (include/rtmi_gather.h): the device draws spp directions per point, traces one
        radiance() path along each and reduces per point; no ray is built on the host.  mode "cosine": points and normals
        [n, 3] (any length), value = the irradiance E = pi * mean over cosine-distributed directions.  mode "sphere":
        points only, value = the mean radiance over uniform directions and, with sh=True, sh [n, 9, 3]: its projection on
        the real spherical harmonics of bands 0..2 (sh_irradiance convolves it).  Path (i, s) is radiance()'s of the ray
        (points[i], gather_directions(...)[i, s]) with first_ray = first_point + i, first_sample + s, stream_skip = 0,
        t_min = path_t_min = t_min, bit for bit.  slab_points: points traced per launch (0: 256 MiB of samples); no output bit
        depends on it.  Returns dict(value f32 [n, 3], stderr f32 [n, 3] (+inf for spp = 1), kernel_ms[, sh]).
        With torch tensors on the scene's device the call is enqueued on torch's current stream (rtmi_gather_device) and
        returns torch tensors on that device: no host copy is made; its per-sample scratch is a torch allocation of
        scratch_bytes (default: one slab's).  A scene resident on a device list raises Unsupported.
        coop=True (RTMI_FLAG_BATCH_COOP): as in radiance(), same bits on the wave-cooperative kernel."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        if mode not in abi.GATHER_MODES:
            raise ValueError("mode must be one of %s" % ", ".join(sorted(abi.GATHER_MODES)))
        cosine = mode == "cosine"
        if cosine and normals is None:
            raise ValueError("mode 'cosine' needs normals")
        self._ready({}, lights=estimator in ("nee", "env_nee"))
        n, spp = int(points.shape[0]), int(spp)
        want_sh = bool(sh) and not cosine
        p = abi.GatherParams(n, spp, abi.GATHER_MODES[mode], abi.ROULETTE_ESTIMATORS[estimator], _batch_coop_flags(flags, coop), int(max_depth),
                             float(t_min), int(seed) & (2 ** 64 - 1), int(first_point) & (2 ** 64 - 1), int(first_sample),
                             int(slab_points), float(env_select_p))
        if hasattr(points, "data_ptr") and hasattr(points, "is_cuda"):
            return self._gather_torch(p, points, normals if cosine else None, times, want_sh, scratch_bytes)
        pts = np.ascontiguousarray(points, dtype=np.float32)
        nrm = np.ascontiguousarray(normals, dtype=np.float32) if cosine else None
        if pts.ndim != 2 or pts.shape[1] != 3 or (cosine and nrm.shape != pts.shape):
            raise ValueError("points and normals are [n, 3] arrays")
        tm = None if times is None else np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float32), (n,)))
        ms = C.c_double(0.0)
        res = {"value": np.zeros((n, 3), np.float32), "stderr": np.zeros((n, 3), np.float32)}
        if want_sh:
            res["sh"] = np.zeros((n, 9, 3), np.float32)
        self.host._check(self.host.lib.rth_gather(self.h, C.byref(p), pts.ctypes.data, nrm.ctypes.data if cosine else None,
                                                   None if tm is None else tm.ctypes.data, res["value"].ctypes.data,
                                                   res["stderr"].ctypes.data, res["sh"].ctypes.data if want_sh else None,
                                                   C.byref(ms)))
        res["kernel_ms"] = ms.value
        return res

    def _gather_torch(self, p, points, normals, times, want_sh, scratch_bytes):
        import torch

        dev = points.device
        if dev.type != "cuda" or (dev.index or 0) != self.device:
            raise ValueError("the points are on %s, the scene is on device %d" % (dev, self.device))
        for a in (points,) if normals is None else (points, normals):
            if a.dtype != torch.float32 or a.dim() != 2 or a.shape != (p.n, 3) or a.device != dev:
                raise ValueError("points and normals are float32 [n, 3] tensors on one device")
        pts = points.contiguous()
        nrm = None if normals is None else normals.contiguous()
        tm = None if times is None else torch.as_tensor(times, dtype=torch.float32, device=dev).expand(p.n).contiguous()
        if scratch_bytes is None:  # one slab of the host form's size, or the whole batch if that is smaller
            slab = p.slab_points or max((256 << 20) // (12 * max(p.spp, 1)), 1)
            scratch_bytes = 12 * max(p.spp, 1) * max(min(slab, p.n), 1)
        scratch_bytes = int(scratch_bytes)
        scratch = torch.empty(((scratch_bytes + 3) // 4,), dtype=torch.float32, device=dev)
        res = {"value": torch.empty((p.n, 3), dtype=torch.float32, device=dev),
               "stderr": torch.empty((p.n, 3), dtype=torch.float32, device=dev)}
        if want_sh:
            res["sh"] = torch.empty((p.n, 9, 3), dtype=torch.float32, device=dev)
        # every check of the entry is made for an empty batch too; it then launches nothing
        self.host._check(self.host.lib.rth_gather_device(
            self.h, C.byref(p), C.c_void_p(pts.data_ptr()), C.c_void_p(nrm.data_ptr()) if nrm is not None else None,
            C.c_void_p(tm.data_ptr()) if tm is not None else None, C.c_void_p(res["value"].data_ptr()),
            C.c_void_p(res["stderr"].data_ptr()), C.c_void_p(res["sh"].data_ptr()) if want_sh else None,
            C.c_void_p(scratch.data_ptr()), C.c_uint64(scratch_bytes), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return res  # scratch returns to torch's allocator, which hands it out again on this stream only behind the kernels

    def render_pixels(self, cam, nx, ny, pixels, ns, estimator="plain", seed=42, first_sample=0, samples=False, env_select_p=0.5,
                      coop=False, count=None, **kw):
        """Chosen pixels of the nx x ny image under `cam` with the render's own paths (include/rtmi_sparse.h).  pixels: an
        integer array of indices row * nx + i into the image's planes (row 0 the top row), or an [n, 2] array of (i, row); it may
        be unsorted and may repeat a pixel.  Sample s
        of entry k is, bit for bit, sample first_sample + s of that pixel in render (estimator "plain"), render_nee ("nee")
        or render_env ("env": nee=False, "env_nee": nee=True with env_select_p) under `seed`: a camera with a lens included.
        kw: flags, max_depth, t_min of default_params.  Returns dict(mean f32 [n, 3], stderr f32 [n, 3] (+inf for ns = 1),
        kernel_ms[, samples f32 [n, ns, 3]]): with first_sample = 0 mean and stderr are the render's linear and stderr
        planes at those pixels.  With a torch tensor on the scene's device the call is enqueued on torch's current stream
        (rtmi_sparse_render_device) and returns torch tensors on that device, samples always among them: no host copy is
        made; count: with a torch list, an int32 tensor on the device whose first word is the number of entries to trace,
        at most the list's length (the d_count of rtmi_sparse_render_device).  A scene resident on a device list raises
        Unsupported.
        coop=True (RTMI_FLAG_BATCH_COOP): as in radiance(), same bits on the wave-cooperative kernel."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        kw["flags"] = _batch_coop_flags(kw.get("flags", 0), coop)
        p = default_params(nx, ny, 1, seed=seed, **kw)
        if hasattr(pixels, "data_ptr") and hasattr(pixels, "is_cuda"):
            return self._render_pixels_torch(cam, p, pixels, int(ns), estimator, int(first_sample), float(env_select_p), count)
        if count is not None:
            raise ValueError("count belongs to a torch list of pixels")
        px = np.asarray(pixels)
        if px.ndim == 2 and px.shape[1] == 2:
            px = px[:, 1].astype(np.int64) * nx + px[:, 0].astype(np.int64)
        if px.ndim != 1 or (px.size and not np.issubdtype(px.dtype, np.integer)):
            raise ValueError("pixels is an integer array of indices or an [n, 2] array of (i, row)")
        if px.size and (px.min() < 0 or px.max() >= 2 ** 32):
            raise ValueError("a pixel index is negative or does not fit 32 bits")
        px = np.ascontiguousarray(px, dtype=np.uint32)
        n = px.shape[0]
        sp = abi.SparseParams(n, int(ns), int(first_sample), abi.ROULETTE_ESTIMATORS[estimator], float(env_select_p))
        ms = C.c_double(0.0)
        res = {"mean": np.zeros((n, 3), np.float32), "stderr": np.zeros((n, 3), np.float32)}
        if samples:
            res["samples"] = np.zeros((n, max(int(ns), 0), 3), np.float32)
        self.host._check(self.host.lib.rth_sparse_render(self.h, cam.h, C.byref(p), C.byref(sp), px.ctypes.data, res["mean"].ctypes.data,
                                                          res["stderr"].ctypes.data, res["samples"].ctypes.data if samples else None,
                                                          C.byref(ms)))
        res["kernel_ms"] = ms.value
        return res

    def _render_pixels_torch(self, cam, p, pixels, ns, estimator, first_sample, env_select_p, count=None):
        import torch

        dev = pixels.device
        if dev.type != "cuda" or (dev.index or 0) != self.device:
            raise ValueError("the pixels are on %s, the scene is on device %d" % (dev, self.device))
        if pixels.is_floating_point() or pixels.dim() not in (1, 2) or (pixels.dim() == 2 and pixels.shape[1] != 2):
            raise ValueError("pixels is an integer tensor of indices or an [n, 2] tensor of (i, row)")
        if pixels.dim() == 2:
            pixels = pixels[:, 1].to(torch.int64) * p.nx + pixels[:, 0].to(torch.int64)
        px = pixels.to(torch.int32).contiguous()  # the words of a uint32 list
        n = px.shape[0]
        sp = abi.SparseParams(n, ns, first_sample, abi.ROULETTE_ESTIMATORS[estimator], env_select_p)
        res = {"mean": torch.empty((n, 3), dtype=torch.float32, device=dev), "stderr": torch.empty((n, 3), dtype=torch.float32, device=dev),
               "samples": torch.empty((n, ns, 3), dtype=torch.float32, device=dev)}
        scratch = torch.empty((4,), dtype=torch.int32, device=dev)
        # every check of the entry is made for an empty list too; it then launches nothing
        self.host._check(self.host.lib.rth_sparse_render_device(
            self.h, cam.h, C.byref(p), C.byref(sp), C.c_void_p(px.data_ptr()), C.c_void_p(count.data_ptr()) if count is not None else None,
            C.c_void_p(res["mean"].data_ptr()), C.c_void_p(res["stderr"].data_ptr()), C.c_void_p(res["samples"].data_ptr()),
            C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return res  # px and scratch return to torch's allocator, which hands them out again on this stream behind the kernels

    def refine_pixels(self, cam, planes, classes=(3,), ns=4, estimator="plain", seed=42, budget=None, mark=4, first_sample=0,
                      env_select_p=0.5, coop=False, **kw):
        """Traces again the pixels of an image whose class is in `classes` and patches the results in (select -> sparse
        render -> patch of include/rtmi_sparse.h, one native call).  planes: a dict with linear f32 [ny,nx,3], rgb8 u8
        [ny,nx,3] and cls u8 [ny,nx], as Upscaler.render returns it (a stderr f32 [ny,nx,3] plane, when present, is patched
        with the new standard errors).  A selected pixel gets render_pixels' mean of ns samples under `seed` (the bits of
        the estimator's full render of ns samples at that pixel), its quantised rgb8, and cls = mark; no other element
        changes.  budget: the most pixels to trace, the first in index order (None: every pixel of the image may be; the
        scratch grows with it: 28 + 12 * ns bytes per pixel of budget).  torch tensors on the scene's device are patched in
        place on torch's current stream, without a host copy; numpy planes are left alone and patched copies returned.
        Returns the dict with refined = (pixels patched, pixels selected).
        coop=True (RTMI_FLAG_BATCH_COOP): as in radiance(), same bits on the wave-cooperative kernel."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        mask = _sparse_mask(classes)
        cls = planes["cls"]
        ny, nx = int(cls.shape[0]), int(cls.shape[1])
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        kw["flags"] = _batch_coop_flags(kw.get("flags", 0), coop)
        p = default_params(nx, ny, 1, seed=seed, **kw)
        cap = nx * ny if budget is None else int(budget)
        sp = abi.SparseParams(cap, int(ns), int(first_sample), abi.ROULETTE_ESTIMATORS[estimator], float(env_select_p))
        names = [n for n in ("linear", "rgb8", "stderr") if planes.get(n) is not None]
        torch_in = hasattr(cls, "data_ptr") and hasattr(cls, "is_cuda")
        want = {"cls": (ny, nx), "linear": (ny, nx, 3), "rgb8": (ny, nx, 3), "stderr": (ny, nx, 3)}
        out = dict(planes)
        if torch_in:
            import torch

            dev = cls.device
            if dev.type != "cuda" or (dev.index or 0) != self.device:
                raise ValueError("the planes are on %s, the scene is on device %d" % (dev, self.device))
            kinds = {"cls": torch.uint8, "rgb8": torch.uint8, "linear": torch.float32, "stderr": torch.float32}
            for n in ["cls"] + names:
                a = planes[n]
                if a.dtype != kinds[n] or tuple(a.shape) != want[n] or a.device != dev or not a.is_contiguous():
                    raise ValueError("plane %r must be a contiguous %s tensor of shape %r on the scene's device" % (n, kinds[n], want[n]))
            nbytes = int(abi.load_rtmi().rtmi_sparse_scratch_bytes(nx * ny, max(cap, 0), max(int(ns), 0)))
            scratch = torch.empty(((nbytes + 15) // 16, 4), dtype=torch.int32, device=dev)
            counts = torch.zeros((2,), dtype=torch.int32, device=dev)
            ptr = {n: C.c_void_p(planes[n].data_ptr()) for n in names}
            self.host._check(self.host.lib.rth_sparse_refine(
                self.h, cam.h, C.byref(p), C.byref(sp), mask, int(mark), C.c_void_p(cls.data_ptr()), ptr.get("linear"), ptr.get("rgb8"),
                ptr.get("stderr"), C.c_void_p(scratch.data_ptr()), C.c_uint64(nbytes), C.c_void_p(counts.data_ptr()), 1,
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            c = counts.cpu().numpy().view(np.uint32)  # the one read-back, for the caller's eyes only
        else:
            kinds = {"cls": np.uint8, "rgb8": np.uint8, "linear": np.float32, "stderr": np.float32}
            for n in ["cls"] + names:
                a = np.asarray(planes[n])
                if a.dtype != kinds[n] or a.shape != want[n]:
                    raise ValueError("plane %r must be a %s array of shape %r" % (n, np.dtype(kinds[n]).name, want[n]))
                out[n] = np.array(a, order="C", copy=True)
            c = np.zeros(2, np.uint32)
            ptr = {n: out[n].ctypes.data for n in names}
            self.host._check(self.host.lib.rth_sparse_refine(
                self.h, cam.h, C.byref(p), C.byref(sp), mask, int(mark), out["cls"].ctypes.data, ptr.get("linear"), ptr.get("rgb8"),
                ptr.get("stderr"), None, 0, c.ctypes.data, 0, None))
        out["refined"] = (int(c[0]), int(c[1]))
        return out

    def render_pixelwise(self, cam, nx, ny, ns, min_spp, step_spp, abs_tol=0.0, rel_tol=0.0, estimator="plain", seed=0, pass_spp=0,
                         out="numpy", env_select_p=0.5, coop=False, **kw):
        """Adaptive sampling per pixel, driven from the device (include/rtmi_pixelwise.h): every pixel gets min_spp samples,
        then step_spp more per step while, in some channel, its stderr > abs_tol + rel_tol * |mean|, up to ns (the last step
        shortened to land on ns).  Each pixel is tested alone, where render_adaptive tests 8x8 tiles, and no step waits for
        the host.  A pixel with spp = n is bit for bit, in linear, rgb8 and stderr, that pixel of render_adaptive(min_spp=n,
        ns=n) (estimator "plain"), render_nee(ns=n) ("nee") or render_env(ns=n) ("env": nee=False, "env_nee": nee=True with
        env_select_p) under `seed`.  pass_spp: at most this many samples per pixel in one launch (0: a whole step; the
        per-sample buffer takes 12 * nx * ny * pass_spp bytes; the result does not depend on it).  kw: flags, max_depth,
        t_min of default_params.  Returns dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], stderr f32 [ny,nx,3], spp u32
        [ny,nx], counts u32 [steps,2], samples): row k of counts is (written, selected) of step k's select, the pixels that
        step traced; samples is the number of paths traced.  out="torch": the device form on torch's current stream; the
        planes, counts (int32 words) and the scratch are torch tensors on the scene's device, nothing is copied to the host,
        and samples is a function that reads counts back when called.  A scene resident on a device list raises
        Unsupported.
        coop=True (RTMI_FLAG_BATCH_COOP, include/rtmi_batch_coop.h): the steps' paths trace on the wave-cooperative kernel
        where the scene allows it, the same bits in every plane, spp and counts included; with out="numpy" the dict gains
        "kernel", rtmi_stats.kernel of the blocking form (abi.RTMI_KERNEL_*)."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        if out not in ("numpy", "torch"):
            raise ValueError('out must be "numpy" or "torch"')
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        kw["flags"] = _batch_coop_flags(kw.get("flags", 0), coop)
        p = default_params(nx, ny, ns, seed=seed, **kw)
        o = abi.PixelwiseOpts(int(min_spp), int(step_spp), abi.ROULETTE_ESTIMATORS[estimator], int(pass_spp), float(abs_tol),
                              float(rel_tol), float(env_select_p))
        lib = abi.load_rtmi()
        steps = int(lib.rtmi_pixelwise_steps(p.ns, o.min_spp, o.step_spp))
        rows = max(steps, 1)  # refused arguments (0 steps) reach the native entry, which names what is wrong
        per_step = np.array([o.min_spp] + [min(o.step_spp, p.ns - n) for n in range(o.min_spp, p.ns, max(o.step_spp, 1))], np.uint64)
        if out == "numpy":
            res, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr", "spp"))
            counts = np.zeros((rows, 2), np.uint32)
            self.host._check(self.host.lib.rth_render_pixelwise(self.h, cam.h, C.byref(p), C.byref(o), *outs[:-1], counts.ctypes.data,
                                                                 outs[-1]))
            st = res.pop("stats")
            res["counts"] = counts[:steps]
            res["samples"] = int(st.samples)
            if coop:
                res["kernel"] = int(st.kernel)
            return res
        import torch

        dev = torch.device("cuda", self.device)
        step = max(o.min_spp, min(o.step_spp, max(p.ns - o.min_spp, 0)))
        nbytes = int(lib.rtmi_pixelwise_scratch_bytes(nx * ny, step if o.pass_spp == 0 or o.pass_spp > step else o.pass_spp, steps))
        res = {"linear": torch.empty((ny, nx, 3), dtype=torch.float32, device=dev), "rgb8": torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev),
               "stderr": torch.empty((ny, nx, 3), dtype=torch.float32, device=dev), "spp": torch.empty((ny, nx), dtype=torch.int32, device=dev),
               "counts": torch.empty((rows, 2), dtype=torch.int32, device=dev)}
        scratch = torch.empty(((nbytes + 15) // 16, 4), dtype=torch.int32, device=dev)
        self.host._check(self.host.lib.rth_render_pixelwise_device(
            self.h, cam.h, C.byref(p), C.byref(o), *[C.c_void_p(res[n].data_ptr()) for n in ("linear", "rgb8", "stderr", "spp", "counts")],
            C.c_void_p(scratch.data_ptr()), C.c_uint64(nbytes), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        counts = res["counts"] = res["counts"][:steps]
        res["samples"] = lambda: int((counts[:, 0].cpu().numpy().astype(np.uint64) * per_step[:steps]).sum())
        return res  # scratch returns to torch's allocator, which hands it out again on this stream only behind the kernels

    def render_windowed(self, cam, nx, ny, ns, min_spp, step_spp, radius=1, abs_tol=0.0, rel_tol=0.0, estimator="plain", seed=0,
                        pass_spp=0, out="numpy", env_select_p=0.5, coop=False, **kw):
        """Adaptive sampling per pixel with a neighbourhood stopping rule, driven from the device (include/rtmi_window.h):
        render_pixelwise's lattice, samples and own-pixel test, but a pixel stays alive while any pixel within the Chebyshev
        radius `radius` of it (the window clipped at the image border) still fails its test below the cap.  radius=0 is
        render_pixelwise bit for bit; a larger radius only adds samples, at every pixel; radius >= max(nx, ny) - 1 stops every
        pixel at the same count (radius is at most abi.RTMI_WINDOW_MAX_RADIUS).  A pixel with spp = n is bit for bit the
        estimator's fixed render at ns = n, as in render_pixelwise.  No inclusion holds against render_adaptive's 8x8 tiles.
        The other arguments, out="torch", coop=True and the returned dict are render_pixelwise's."""
        if estimator not in abi.ROULETTE_ESTIMATORS:
            raise ValueError("estimator must be one of %s" % ", ".join(sorted(abi.ROULETTE_ESTIMATORS)))
        if out not in ("numpy", "torch"):
            raise ValueError('out must be "numpy" or "torch"')
        self._ready(kw, lights=estimator in ("nee", "env_nee"))
        kw["flags"] = _batch_coop_flags(kw.get("flags", 0), coop)
        p = default_params(nx, ny, ns, seed=seed, **kw)
        o = abi.WindowOpts(int(min_spp), int(step_spp), abi.ROULETTE_ESTIMATORS[estimator], int(pass_spp), float(abs_tol),
                           float(rel_tol), float(env_select_p), int(radius))
        lib = abi.load_rtmi()
        steps = int(lib.rtmi_window_steps(p.ns, o.min_spp, o.step_spp))
        rows = max(steps, 1)  # refused arguments (0 steps) reach the native entry, which names what is wrong
        per_step = np.array([o.min_spp] + [min(o.step_spp, p.ns - n) for n in range(o.min_spp, p.ns, max(o.step_spp, 1))], np.uint64)
        if out == "numpy":
            res, outs = _outputs(ny, nx, ("linear", "rgb8", "stderr", "spp"))
            counts = np.zeros((rows, 2), np.uint32)
            self.host._check(self.host.lib.rth_render_window(self.h, cam.h, C.byref(p), C.byref(o), *outs[:-1], counts.ctypes.data,
                                                              outs[-1]))
            st = res.pop("stats")
            res["counts"] = counts[:steps]
            res["samples"] = int(st.samples)
            if coop:
                res["kernel"] = int(st.kernel)
            return res
        import torch

        dev = torch.device("cuda", self.device)
        step = max(o.min_spp, min(o.step_spp, max(p.ns - o.min_spp, 0)))
        nbytes = int(lib.rtmi_window_scratch_bytes(nx * ny, step if o.pass_spp == 0 or o.pass_spp > step else o.pass_spp, steps))
        res = {"linear": torch.empty((ny, nx, 3), dtype=torch.float32, device=dev), "rgb8": torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev),
               "stderr": torch.empty((ny, nx, 3), dtype=torch.float32, device=dev), "spp": torch.empty((ny, nx), dtype=torch.int32, device=dev),
               "counts": torch.empty((rows, 2), dtype=torch.int32, device=dev)}
        scratch = torch.empty(((nbytes + 15) // 16, 4), dtype=torch.int32, device=dev)
        self.host._check(self.host.lib.rth_render_window_device(
            self.h, cam.h, C.byref(p), C.byref(o), *[C.c_void_p(res[n].data_ptr()) for n in ("linear", "rgb8", "stderr", "spp", "counts")],
            C.c_void_p(scratch.data_ptr()), C.c_uint64(nbytes), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        counts = res["counts"] = res["counts"][:steps]
        res["samples"] = lambda: int((counts[:, 0].cpu().numpy().astype(np.uint64) * per_step[:steps]).sum())
        return res  # scratch returns to torch's allocator, which hands it out again on this stream only behind the kernels


def window_spread(active, fail, radius, device=0):
    """The stopping rule of include/rtmi_window.h applied once: active'[p] = active[p] != 0 and some fail byte != 0 within the
    Chebyshev radius of p, the window clipped at the border; bytes 1 or 0.  active, fail: uint8 [ny, nx], both numpy arrays
    (a new array is returned; the kernel runs on `device`, blocking) or both torch tensors on one GPU (active is updated in
    place on torch's current stream and returned; nothing is copied to the host)."""
    lib = abi.load_rtmi()

    def refuse(rc):
        if rc:
            raise ValueError((lib.rtmi_last_error() or b"window_spread failed").decode())

    if isinstance(active, np.ndarray) or isinstance(fail, np.ndarray):
        a, f = np.array(active, np.uint8, order="C", copy=True), np.ascontiguousarray(fail, np.uint8)
        if a.ndim != 2 or a.shape != f.shape:
            raise ValueError("active and fail must be uint8 arrays of one shape [ny, nx]")
        refuse(lib.rtmi_probe_window_spread(int(device), a.shape[1], a.shape[0], int(radius), a.ctypes.data, f.ctypes.data))
        return a
    import torch

    if not (active.is_cuda and fail.device == active.device and active.dtype == fail.dtype == torch.uint8 and active.dim() == 2
            and active.shape == fail.shape and active.is_contiguous() and fail.is_contiguous()):
        raise ValueError("active and fail must be contiguous uint8 tensors of one shape [ny, nx] on one GPU")
    with torch.cuda.device(active.device):
        refuse(lib.rtmi_window_spread_device(C.c_void_p(active.data_ptr()), C.c_void_p(fail.data_ptr()), active.shape[1], active.shape[0],
                                             int(radius), C.c_void_p(torch.cuda.current_stream(active.device).cuda_stream)))
    return active


IRRADIANCE_STREAM = 5  # the Philox stream id of irradiance()'s directions (0 path, 2 scene, 3 light samples, 4 roulette)


def irradiance_directions(normals, spp, seed=0):
    """Scene.irradiance's directions: float32 [n, spp, 3], unit length, cosine-distributed about each normal.  Direction
    k of point i takes words 0 and 1 of the Philox block with counter (0, k, i, IRRADIANCE_STREAM) under the key `seed`
    as 24-bit uniforms u1, u2 (philox.py): r = sqrt(u1), phi = 2 pi u2, (r cos phi, r sin phi, sqrt(1 - u1)) in an
    orthonormal frame around the normal.  Host code: needs no GPU."""
    from . import philox

    nrm = np.asarray(normals, dtype=np.float64)
    n = nrm.shape[0]
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    # the frame: the world axis least aligned with the normal, made orthogonal to it
    axis = np.eye(3)[np.argmin(np.abs(nrm), axis=1)]
    t = np.cross(axis, nrm)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    kk, ii = np.meshgrid(np.arange(spp, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    w = philox.philox4x32_10_np(np.zeros_like(kk), kk, ii, np.full_like(kk, IRRADIANCE_STREAM), seed)
    u1 = (w[0] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    x, y, z = r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u1)
    d = x[..., None] * t[:, None, :] + y[..., None] * b[:, None, :] + z[..., None] * nrm[:, None, :]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return np.ascontiguousarray(d.astype(np.float32))


def gather_directions(normals, spp, seed=0, mode="cosine", first_point=0, first_sample=0, n=None):
    """Scene.gather's directions (rtmi_gather_directions, include/rtmi_gather.h): float32 [n, spp, 3], computed on the host
    by the inline functions the kernels compile.  mode "cosine": about each of normals [n, 3]; mode "sphere": uniform, for n
    points (normals is not read).  Needs no GPU."""
    if mode not in abi.GATHER_MODES:
        raise ValueError("mode must be one of %s" % ", ".join(sorted(abi.GATHER_MODES)))
    nrm = None
    if mode == "cosine":
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] != 3:
            raise ValueError("normals is an [n, 3] array, not %r" % (nrm.shape,))
        n = nrm.shape[0]
    elif n is None:
        n = int(np.asarray(normals).shape[0])
    p = abi.GatherParams(int(n), int(spp), abi.GATHER_MODES[mode], 0, 0, 1, 0.001, int(seed) & (2 ** 64 - 1),
                         int(first_point) & (2 ** 64 - 1), int(first_sample), 0, 0.5)
    out = np.zeros((int(n), max(int(spp), 0), 3), np.float32)
    lib = abi.load_rtmi()
    if lib.rtmi_gather_directions(C.byref(p), None if nrm is None else nrm.ctypes.data, int(n), out.ctypes.data):
        raise ValueError((lib.rtmi_last_error() or b"").decode())
    return out


SH_COSINE_LOBE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)  # A_l of bands 0..2: the clamped-cosine kernel's zonal factors


def sh_basis(directions):
    """The nine real spherical harmonics of include/rtmi_gather.h at unit directions [..., 3], float64 [..., 9]."""
    d = np.asarray(directions, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2, c20, c22 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c20 * (3.0 * z * z - 1.0), c2 * x * z,
                     c22 * (x * x - y * y)], axis=-1)


def sh_irradiance(sh, normals):
    """Irradiance from SH probes (Ramamoorthi and Hanrahan 2001): sh [n, 9, 3] of Scene.gather(mode="sphere"), normals
    [n, 3] (any length) -> float64 [n, 3]: sum_k A_band(k) sh[k] Y_k(normal), the probe's radiance convolved with the
    cosine lobe A = (pi, 2 pi / 3, pi / 4).  numpy."""
    sh = np.asarray(sh, np.float64)
    nrm = np.asarray(normals, np.float64)
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    a = np.array([SH_COSINE_LOBE[0]] + [SH_COSINE_LOBE[1]] * 3 + [SH_COSINE_LOBE[2]] * 5)
    return np.einsum("...k,...kc->...c", sh_basis(nrm) * a, sh)


# rtmi_light_node and rtmi_light_path (include/rtmi_light_tree.h) as numpy sees them
LIGHT_NODE_DTYPE = np.dtype([("c", "<f4", (3,)), ("r2", "<f4"), ("power", "<f4"), ("link", "<u4"), ("pad", "<u4", (2,))])
LIGHT_PATH_DTYPE = np.dtype([("trail", "<u4"), ("depth", "<u4")])

# rtmi_ray and rtmi_hit (include/rtmi_query.h) as numpy sees them
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("t_min", "<f4"), ("d", "<f4", (3,)), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("p", "<f4", (3,)), ("n", "<f4", (3,)), ("item", "<i4"),
                      ("prim", "<i4"), ("material", "<i4")])


def primary_rays(cam, nx, ny):
    """The pixel-centre rays of a camera from its lens centre, for picking and timing: (origins, directions), float32
    [ny, nx, 3] each, row 0 the top row.  cam: a Camera of Host or its lowered form (abi.Camera).  Pixel (column i, row j
    from the bottom) looks along ((llc + horizontal * u) + vertical * v) - origin with u = (i + 0.5) / nx and
    v = (j + 0.5) / ny, in float32 as the device's camera_sample computes a direction."""
    c = cam.lower() if hasattr(cam, "lower") else cam
    f32 = np.float32
    llc, hor, ver, org = (np.array(list(x), f32) for x in (c.lower_left_corner, c.horizontal, c.vertical, c.origin))
    u = ((np.arange(nx, dtype=f32) + f32(0.5)) / f32(nx)).astype(f32)
    v = ((np.arange(ny, dtype=f32)[::-1] + f32(0.5)) / f32(ny)).astype(f32)
    d = ((llc + hor * u[None, :, None]) + ver * v[:, None, None]) - org
    return np.ascontiguousarray(np.broadcast_to(org, (ny, nx, 3))), np.ascontiguousarray(d.astype(f32))


# the output planes of the render methods: channels after [ny, nx], dtype
_PLANES = {"linear": ((3,), np.float32), "rgb8": ((3,), np.uint8), "stderr": ((3,), np.float32), "spp": ((), np.uint32),
           "bounces": ((), np.uint32), "albedo": ((3,), np.float32), "normal": ((3,), np.float32), "depth": ((), np.float32),
           "hits": ((), np.uint32)}


def _rtmi_check(lib, rc, what):
    """Raises for a refusal of librtmi's entry `what`: Unsupported for RTMI_ERR_UNSUPPORTED, HostError otherwise."""
    if rc != 0:
        raise {2: Unsupported}.get(rc, HostError)("%s failed (%d): %s" % (what, rc, lib.rtmi_last_error().decode()))


def _check_plane(name, a, want, f32=np.float32):
    """The shape and dtype checks of an input plane (a numpy array, or a torch tensor with f32 = torch.float32)."""
    if tuple(a.shape) != want:
        raise ValueError("%s must have the shape %r, not %r" % (name, want, tuple(a.shape)))
    if a.dtype != f32:
        raise ValueError("%s must be float32, not %s" % (name, a.dtype))


def _feature_planes(ny, nx, linear, albedo, normal, depth, stderr):
    """The inputs of denoise() and Temporal.push() by name, checked, as contiguous arrays; stderr only when given."""
    planes = {"linear": linear, "albedo": albedo, "normal": normal, "depth": depth}
    if stderr is not None:
        planes["stderr"] = stderr
    for name, a in planes.items():
        a = np.asarray(a)
        _check_plane(name, a, (ny, nx) if name == "depth" else (ny, nx, 3))
        planes[name] = np.ascontiguousarray(a)
    return planes


class _Handle:
    """What the handle classes share: h (None once closed), the list of open handles that Host.free_all() closes, close()
    and the context manager.  A subclass names itself in _closed ("the ... is closed") and frees h in _destroy."""
    h = None

    def _opened(self, h, registry):
        self.h, self._open = h, registry
        registry.append(self)

    def _check(self, rc, what):  # the handles of librtmi's own entries; the others go through Host._check
        _rtmi_check(self.lib, rc, what)

    def _handle(self):
        if not self.h:
            raise HostError("the %s is closed" % self._closed)
        return self.h

    def close(self):
        if self.h:
            h, self.h = self.h, None
            if self in self._open:
                self._open.remove(self)
            self._destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Session(_Handle):
    """A render session of Scene.session (include/rtmi_session.h).  Calls on it serialise with every other call on its
    scene.  close() frees its device state (76 B per tile-padded pixel); Host.free_all() closes what is still open."""

    _closed = "session"

    def __init__(self, host, h, nx, ny, keep=()):
        self.host, self.nx, self.ny, self.keep = host, nx, ny, keep
        self._opened(h, host.__dict__.setdefault("_sessions", []))

    def _destroy(self, h):
        self.host._check(self.host.lib.rth_session_close(h))

    def render(self, spp):
        """FIXED sessions: spp more samples for every tile.  Returns the call's stats."""
        st = abi.Stats()
        self.host._check(self.host.lib.rth_session_render(self._handle(), spp, C.byref(st)))
        return _stats(st)

    def refine(self, abs_tol, rel_tol, cap):
        """REFINE sessions: advance to the noise target under the cap; a call may tighten, never loosen.  The image then
        equals render_adaptive's (or render_adaptive_roulette's) with this call's arguments, and no sample was traced
        twice.  Returns the call's stats (samples = the paths this call traced)."""
        st = abi.Stats()
        self.host._check(self.host.lib.rth_session_refine(self._handle(), abs_tol, rel_tol, cap, C.byref(st)))
        return _stats(st)

    def image(self):
        """The session as it stands: dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], stderr f32 [ny,nx,3], spp u32 [ny,nx],
        bounces u32 [ny,nx] (zeros without roulette))."""
        out = {n: np.zeros((self.ny, self.nx) + _PLANES[n][0], _PLANES[n][1]) for n in ("linear", "rgb8", "stderr", "spp", "bounces")}
        self.host._check(self.host.lib.rth_session_image(self._handle(), *[a.ctypes.data for a in out.values()]))
        return out

    def spp(self):
        """(min, max) of the tiles' sample counts."""
        lo, hi = C.c_uint32(0), C.c_uint32(0)
        self.host._check(self.host.lib.rth_session_spp(self._handle(), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def save(self):
        """The session as a blob (bytes; the layout is in include/rtmi_session.h)."""
        need = C.c_size_t(0)
        self.host._check(self.host.lib.rth_session_export(self._handle(), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self.host._check(self.host.lib.rth_session_export(self._handle(), buf, need.value, C.byref(need)))
        return buf.raw

    def load(self, blob):
        """Restores a blob of save() into this session, which must have the same identity (HostError otherwise, the
        session unchanged); clears the failed state."""
        blob = bytes(blob)
        self.host._check(self.host.lib.rth_session_import(self._handle(), blob, len(blob)))

    def merge(self, other):
        """Takes in the samples of `other`, a FIXED session of equal identity whose range starts where this one's ends."""
        self.host._check(self.host.lib.rth_session_merge(self._handle(), other._handle()))

    def render_for(self, seconds, step_spp):
        """render(step_spp) until the wall clock passes `seconds` (at least one step).  Returns the spp reached."""
        import time

        t0 = time.monotonic()
        while True:
            self.render(step_spp)
            if time.monotonic() - t0 >= seconds:
                return self.spp()[1]


# the planes of rtmi_frame_out in Frame.render's result: (group, name in the group, field, channels, dtype)
_FRAME_PLANES = ((None, "linear", "linear", (3,), "float32"), (None, "rgb8", "rgb8", (3,), "uint8"),
                 ("noisy", "linear", "noisy_linear", (3,), "float32"), ("noisy", "stderr", "noisy_stderr", (3,), "float32"),
                 ("features", "albedo", "albedo", (3,), "float32"), ("features", "normal", "normal", (3,), "float32"),
                 ("features", "depth", "depth", (), "float32"), ("features", "hits", "hits", (), "uint32"),
                 ("accumulated", "linear", "accum_linear", (3,), "float32"), ("accumulated", "stderr", "accum_stderr", (3,), "float32"),
                 ("accumulated", "history", "history", (), "float32"), ("accumulated", "motion", "motion", (2,), "float32"))


class Frame(_Handle):
    """A frame handle of Scene.frame (include/rtmi_frame.h).  Calls on it serialise with every other call on its scene.
    close() frees its device memory (227 B per pixel with every stage on); Host.free_all() closes what is still open.
    Usable as a context manager."""

    _closed = "frame"

    def __init__(self, host, h, nx, ny, device, temporal, keep=()):
        self.host, self.nx, self.ny, self.device, self.temporal, self.keep = host, nx, ny, device, temporal, keep
        self._opened(h, host.__dict__.setdefault("_frames", []))

    def _destroy(self, h):
        self.host._check(self.host.lib.rth_frame_close(h))

    def render(self, cam, ns, seed=0, aux=False, out="numpy", tonemap=None, dt=0.0):
        """One frame under `cam` (a Camera of Host) with ns >= 2 samples per pixel.  Returns dict(linear f32 [ny,nx,3],
        rgb8 u8 [ny,nx,3], stats); aux=True adds render_temporal's noisy = dict(linear, stderr), features = dict(albedo,
        normal, depth, hits) and, with a history, accumulated = dict(linear, stderr, history, motion).  out="numpy": host
        arrays; out="torch": torch tensors on the scene's device, written by the device form without a host copy.
        tonemap: a Tonemap of the frame's size and device (ValueError otherwise); rgb8 is then tonemap.apply(linear, dt)'s,
        through the device form with out="torch" and the host form with out="numpy", and exposure = its state is added."""
        h = self._handle()
        if out not in ("numpy", "torch"):
            raise ValueError("out must be 'numpy' or 'torch'")
        if tonemap is not None and (not isinstance(tonemap, Tonemap) or (tonemap.nx, tonemap.ny, tonemap.device) !=
                                    (self.nx, self.ny, self.device)):
            raise ValueError("tonemap must be a Tonemap of the frame's size (%d x %d) and device (%d)" % (self.nx, self.ny, self.device))
        if out == "torch":
            import torch

            dev = torch.device("cuda", self.device)
        res, ptrs = {}, abi.FrameOut()
        for group, name, field, ch, dtype in _FRAME_PLANES:
            if (group and not aux) or (group == "accumulated" and not self.temporal):
                continue
            shape = (self.ny, self.nx) + ch
            if out == "torch":
                a = torch.empty(shape, dtype=getattr(torch, dtype), device=dev)
                setattr(ptrs, field, a.data_ptr())
            else:
                a = np.zeros(shape, dtype)
                setattr(ptrs, field, a.ctypes.data)
            (res.setdefault(group, {}) if group else res)[name] = a
        st = abi.Stats()
        self.host._check(self.host.lib.rth_frame_render(h, cam.h, ns, int(seed) & (2 ** 64 - 1), C.byref(ptrs),
                                                         1 if out == "torch" else 0, C.byref(st)))
        res["stats"] = _stats(st)
        if tonemap is not None:
            tm = tonemap.apply(res["linear"], dt=dt, sync=True)
            res["rgb8"], res["exposure"] = tm["rgb8"], tm["exposure"]
        return res

    def reset(self):
        """Forgets the frames rendered so far: the next frame starts a fresh history."""
        self.host._check(self.host.lib.rth_frame_reset(self._handle()))


# the planes of rtmi_upscaler_out in Upscaler.render's result: (group, name in the group, field, low size, channels, dtype)
_UPSCALER_PLANES = ((None, "linear", "linear", False, (3,), "float32"), (None, "rgb8", "rgb8", False, (3,), "uint8"),
                    (None, "cls", "cls", False, (), "uint8"),
                    ("guide", "albedo", "albedo", False, (3,), "float32"), ("guide", "normal", "normal", False, (3,), "float32"),
                    ("guide", "depth", "depth", False, (), "float32"),
                    ("low", "linear", "linear", True, (3,), "float32"), ("low", "albedo", "albedo", True, (3,), "float32"),
                    ("low", "normal", "normal", True, (3,), "float32"), ("low", "depth", "depth", True, (), "float32"))


class Upscaler(_Handle):
    """An upscaler handle of Scene.upscaler (include/rtmi_upscale.h): nx x ny images rebuilt from lx x ly frames.  Calls on
    one handle serialise on a lock of its own; a render holds its scene twice (the low frame, then the features and the
    reconstruction), and another render of the scene may run between the two without touching the handle's planes.  close() frees its device memory (the low frame's, 40 B per low pixel
    and 16 B per full pixel); Host.free_all() closes what is still open.  Usable as a context manager."""

    _closed = "upscaler"

    def __init__(self, host, h, nx, ny, lx, ly, device, keep=()):
        self.host, self.nx, self.ny, self.lx, self.ly, self.device, self.keep = host, nx, ny, lx, ly, device, keep
        self._opened(h, host.__dict__.setdefault("_upscalers", []))

    def _destroy(self, h):
        self.host._check(self.host.lib.rth_upscaler_close(h))

    def render(self, cam, ns, seed=0, aux=False, out="numpy", tonemap=None, dt=0.0):
        """One frame under `cam` (a Camera of Host): the low frame with ns >= 2 samples per pixel, rebuilt at the full size.
        Returns dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], cls u8 [ny,nx] (0 background, 1 guided, 2 nearest-similar,
        3 mismatch), stats); aux=True adds guide = dict(albedo, normal, depth) at the full size and low = dict(linear,
        albedo, normal, depth) at the low size: what upscale() takes.  out="numpy": host arrays; out="torch": torch tensors
        on the scene's device, written by the device form without a host copy.  tonemap: a Tonemap of the full size and
        the scene's device (ValueError otherwise); rgb8 is then tonemap.apply(linear, dt)'s, as Frame.render composes it,
        and exposure = its state is added."""
        h = self._handle()
        if out not in ("numpy", "torch"):
            raise ValueError("out must be 'numpy' or 'torch'")
        if tonemap is not None and (not isinstance(tonemap, Tonemap) or (tonemap.nx, tonemap.ny, tonemap.device) !=
                                    (self.nx, self.ny, self.device)):
            raise ValueError("tonemap must be a Tonemap of the full size (%d x %d) and device (%d)" % (self.nx, self.ny, self.device))
        if out == "torch":
            import torch

            dev = torch.device("cuda", self.device)
        res, ptrs = {}, abi.UpscalerOut()
        for group, name, field, low, ch, dtype in _UPSCALER_PLANES:
            if group and not aux:
                continue
            shape = ((self.ly, self.lx) if low else (self.ny, self.nx)) + ch
            if out == "torch":
                a = torch.empty(shape, dtype=getattr(torch, dtype), device=dev)
                addr = a.data_ptr()
            else:
                a = np.zeros(shape, dtype)
                addr = a.ctypes.data
            setattr(ptrs.low if low else ptrs, field, addr)
            (res.setdefault(group, {}) if group else res)[name] = a
        st = abi.Stats()
        self.host._check(self.host.lib.rth_upscaler_render(h, cam.h, ns, int(seed) & (2 ** 64 - 1), C.byref(ptrs),
                                                            1 if out == "torch" else 0, C.byref(st)))
        res["stats"] = _stats(st)
        if tonemap is not None:
            tm = tonemap.apply(res["linear"], dt=dt, sync=True)
            res["rgb8"], res["exposure"] = tm["rgb8"], tm["exposure"]
        return res

    def reset(self):
        """Forgets the frames rendered so far: the next frame starts a fresh history."""
        self.host._check(self.host.lib.rth_upscaler_reset(self._handle()))


def _outputs(ny, nx, names, sig=None):
    """The zeroed planes `names` of a render as its result dict, and the trailing arguments of the native entry: the
    planes' addresses in that order, the path signatures' (u64 [ny,nx]; NULL unless sig; sig=None: the entry takes none;
    the methods that take them pass bool(sig)) and the stats.  _result() completes the dict after the call."""
    out = {n: np.zeros((ny, nx) + _PLANES[n][0], _PLANES[n][1]) for n in names}
    args = [a.ctypes.data for a in out.values()]
    out["stats"] = abi.Stats()
    if sig:
        out["sig"] = np.zeros((ny, nx), np.uint64)
    if sig is not None:
        args.append(out["sig"].ctypes.data if sig else None)
    return out, args + [C.byref(out["stats"])]


def _result(out):
    out["stats"] = _stats(out["stats"])
    return out


def _stats(st):
    return {"kernel_ms": st.kernel_ms, "render_ms": st.render_ms, "samples": int(st.samples), "tiles": st.tiles,
            "chunks": st.chunks, "blocks": st.blocks, "kernel": st.kernel}


class _Camera(_Obj):
    def render(self, world, nx, ny, ns, seed=42, flags=0, device=0, precision="f32"):
        """Camera::render(world, nx, ny, ns): lower + upload + render + free, like one create_image call.
        precision="f64": the f64 render mode (include/rtmi_f64.h); linear is float64."""
        if precision == "f64":  # rth_camera_render_f64: the device handle and its planes are freed after the render
            lin = np.zeros((ny, nx, 3), np.float64)
            rgb = np.zeros((ny, nx, 3), np.uint8)
            st = abi.Stats()
            self.host._check(self.host.lib.rth_camera_render_f64(self.h, world.h, nx, ny, ns, seed, flags, device,
                                                                  lin.ctypes.data, rgb.ctypes.data, C.byref(st)))
            return {"linear": lin, "rgb8": rgb, "stats": _stats(st)}
        if precision != "f32":
            raise ValueError("precision must be 'f32' or 'f64'")
        lin = np.zeros((ny, nx, 3), np.float32)
        rgb = np.zeros((ny, nx, 3), np.uint8)
        st = abi.Stats()
        self.host._check(self.host.lib.rth_camera_render(self.h, world.h, nx, ny, ns, seed, flags, device,
                                                          lin.ctypes.data, rgb.ctypes.data, C.byref(st)))
        return {"linear": lin, "rgb8": rgb, "stats": _stats(st)}

    def get_ray(self, s, t, seed=0):
        out = np.zeros(7)
        self.host._check(self.host.lib.rth_get_ray(self.h, s, t, seed, out.ctypes.data))
        return out

    def state(self):
        out = np.zeros(21)
        self.host._check(self.host.lib.rth_camera_state(self.h, out.ctypes.data))
        return out

    def lower(self):
        c = abi.Camera()
        self.host._check(self.host.lib.rth_camera_lower(self.h, C.byref(c)))
        return c

    def lower_f64(self):
        c = abi.CameraF64()
        self.host._check(self.host.lib.rth_camera_lower_f64(self.h, C.byref(c)))
        return c


class Host:
    PLANE_YZ, PLANE_ZX, PLANE_XY = PLANE_YZ, PLANE_ZX, PLANE_XY
    AXIS_X, AXIS_Y, AXIS_Z = AXIS_X, AXIS_Y, AXIS_Z
    precision = "host"

    def __init__(self):
        self.lib = abi.bind_host_relight(abi.bind_host_update(abi.load_host()))

    def _raise(self):
        msg = (self.lib.rth_last_error() or b"").decode()
        raise {2: Panic, 3: Unsupported}.get(self.lib.rth_last_error_code(), HostError)(msg)

    def _check(self, rc):
        if rc == 0:
            return
        msg = (self.lib.rth_last_error() or b"").decode()
        raise {2: Panic, 3: Unsupported}.get(rc, HostError)(msg)

    def seed_scene_rng(self, seed):
        self.lib.rth_seed_scene_rng(int(seed))

    def free_all(self):
        for ses in list(getattr(self, "_sessions", [])):  # sessions before their scenes
            ses.close()
        for frm in list(getattr(self, "_frames", [])):  # ... and frames
            frm.close()
        for ups in list(getattr(self, "_upscalers", [])):  # ... and upscalers
            ups.close()
        for tmp in list(_temporals):
            tmp.close()
        for tm in list(_tonemaps):
            tm.close()
        self.lib.rth_free_all()

    # ---- textures (src/texture.rs) ----
    def SolidTexture(self, r, g, b):
        return _Obj(self, self.lib.rth_tex_solid(r, g, b))

    def CheckerTexture(self, odd, even):
        return _Obj(self, self.lib.rth_tex_checker(odd.h, even.h), (odd, even))

    def NoiseTexture(self, scale):
        return _Obj(self, self.lib.rth_tex_noise(scale))

    def ImageTexture(self, data, nx, ny):
        arr = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1))
        if arr.size != nx * ny * 3:
            raise Panic("ImageTexture: data size != 3*nx*ny")
        return _Obj(self, self.lib.rth_tex_image(arr.ctypes.data, nx, ny))

    # ---- materials (src/material.rs) ----
    def Lambertian(self, tex):
        return _Obj(self, self.lib.rth_mat_lambertian(tex.h), (tex,))

    def Metal(self, tex, fuzz):
        return _Obj(self, self.lib.rth_mat_metal(tex.h, fuzz), (tex,))

    def Dielectric(self, ref_idx):
        return _Obj(self, self.lib.rth_mat_dielectric(ref_idx))

    def DiffuseLight(self, tex):
        return _Obj(self, self.lib.rth_mat_diffuse_light(tex.h), (tex,))

    def Isotropic(self, tex):
        return _Obj(self, self.lib.rth_mat_isotropic(tex.h), (tex,))

    # ---- hittables ----
    def Sphere(self, center, radius, material):
        c = _d3(center)
        return _Obj(self, self.lib.rth_sphere(c[0], c[1], c[2], radius, material.h), (material,))

    def MovingSphere(self, center0, center1, time0, time1, radius, material):
        a, b = _d3(center0), _d3(center1)
        return _Obj(self, self.lib.rth_moving_sphere(a[0], a[1], a[2], b[0], b[1], b[2], time0, time1, radius,
                                                     material.h), (material,))

    def Rect(self, plane, x0, y0, x1, y1, k, material):
        return _Obj(self, self.lib.rth_rect(plane, x0, y0, x1, y1, k, material.h), (material,))

    def Cube(self, p_min, p_max, material):
        a, b = _d3(p_min), _d3(p_max)
        return _Obj(self, self.lib.rth_cube(a[0], a[1], a[2], b[0], b[1], b[2], material.h), (material,))

    def FlipNormals(self, hittable):
        return _Obj(self, self.lib.rth_flip_normals(hittable.h), (hittable,))

    def Traslate(self, hittable, offset):
        o = _d3(offset)
        return _Obj(self, self.lib.rth_translate(hittable.h, o[0], o[1], o[2]), (hittable,))

    def Rotate(self, axis, hittable, angle):
        return _Obj(self, self.lib.rth_rotate(axis, hittable.h, angle), (hittable,))

    def ConstantMedium(self, boundary, density, texture):
        return _Obj(self, self.lib.rth_constant_medium(boundary.h, density, texture.h), (boundary, texture))

    def HittableList(self):
        return _List(self, self.lib.rth_list_new())

    def BVHNode(self, hittables, time0, time1):
        arr = (C.c_void_p * len(hittables))(*[h.h for h in hittables])
        return _Obj(self, self.lib.rth_bvh(arr, len(hittables), time0, time1), tuple(hittables))

    def Camera(self, look_from, look_at, view_up, vertical_fov, aspect, aperture, focus_dist, time0, time1):
        f, a, u = _d3(look_from), _d3(look_at), _d3(view_up)
        return _Camera(self, self.lib.rth_camera(f[0], f[1], f[2], a[0], a[1], a[2], u[0], u[1], u[2], vertical_fov,
                                                 aspect, aperture, focus_dist, time0, time1))

    # ---- lowering / rendering ----
    def lower(self, world):
        return Scene(self, world)

    def create_image(self, ny, nx, ns, cam, world, seed=42, flags=0, device=0):
        """tests/test.rs:55-85: returns the P3 text (bytes).  Argument order (ny, nx, ns, cam, world)."""
        img = cam.render(world, nx, ny, ns, seed=seed, flags=flags, device=device)
        return ppm_p3(img["rgb8"])

    # ---- CPU evaluation of the mirror (f64) ----
    def hit(self, hittable, origin, direction, time=0.0, t_min=0.001, t_max=float("inf"), seed=0):
        o, d = _d3(origin), _d3(direction)
        out = np.zeros(9)
        found = C.c_int(0)
        tmx = 1.8e308 if t_max == float("inf") else t_max
        tmn = -1.8e308 if t_min == -float("inf") else t_min
        self._check(self.lib.rth_hit(hittable.h, o.ctypes.data, d.ctypes.data, time, tmn, tmx, seed, out.ctypes.data,
                                     C.byref(found)))
        if not found.value:
            return None
        return {"t": out[0], "u": out[1], "v": out[2], "p": out[3:6].copy(), "normal": out[6:9].copy()}

    def bounding_box(self, hittable, t0=0.0, t1=1.0):
        out = np.zeros(6)
        found = C.c_int(0)
        self._check(self.lib.rth_bounding_box(hittable.h, t0, t1, out.ctypes.data, C.byref(found)))
        if not found.value:
            return None
        return out[:3].copy(), out[3:].copy()

    def tex_value(self, tex, u, v, p):
        pp = _d3(p)
        out = np.zeros(3)
        self._check(self.lib.rth_tex_value(tex.h, u, v, pp.ctypes.data, out.ctypes.data))
        return out

    def scatter(self, mat, ray_o, ray_d, time, rec, seed=0):
        o, d = _d3(ray_o), _d3(ray_d)
        r9 = np.ascontiguousarray(np.concatenate([[rec["t"], rec["u"], rec["v"]], rec["p"], rec["normal"]]),
                                  dtype=np.float64)
        out = np.zeros(10)
        sc = C.c_int(0)
        self._check(self.lib.rth_scatter(mat.h, o.ctypes.data, d.ctypes.data, time, r9.ctypes.data, seed,
                                         out.ctypes.data, C.byref(sc)))
        if not sc.value:
            return None
        return {"o": out[0:3].copy(), "d": out[3:6].copy(), "time": out[6], "attenuation": out[7:10].copy()}

    def emitted(self, mat, u, v, p):
        pp = _d3(p)
        out = np.zeros(3)
        self._check(self.lib.rth_emitted(mat.h, u, v, pp.ctypes.data, out.ctypes.data))
        return out

    def color_sample(self, cam, world, nx, ny, i, j, s, seed=42, sky=False, face_forward=False, uv_book=False):
        """color() of one camera sample on the CPU mirror.  Opt-in extensions (off by default): sky = background of
        color.rs:18-20; face_forward = opaque materials see the normal turned against the ray; uv_book = pi/2 in
        get_sphere_uv instead of FRAC_2_PI (sphere.rs:13)."""
        out = np.zeros(3)
        self.lib.rth_set_sky_background(1 if sky else 0)
        self.lib.rth_set_face_forward(1 if face_forward else 0)
        self.lib.rth_set_uv_book(1 if uv_book else 0)
        try:
            self._check(self.lib.rth_color_sample(cam.h, world.h, nx, ny, i, j, s, seed, out.ctypes.data))
        finally:
            self.lib.rth_set_sky_background(0)
            self.lib.rth_set_face_forward(0)
            self.lib.rth_set_uv_book(0)
        return out

    def perlin_tables(self, tex):
        rv = np.zeros(768)
        pm = np.zeros(768, np.int32)
        self._check(self.lib.rth_perlin_tables(tex.h, rv.ctypes.data, pm.ctypes.data))
        return rv.reshape(256, 3), pm.reshape(3, 256)


def release_cached():
    """Returns the per-sample buffers that destroyed handles left parked for their successors (rtmi_release_cached)."""
    abi.load_rtmi().rtmi_release_cached()


def ppm_p3(rgb8):
    """The P3 text of create_image (tests/test.rs:59,79) through the native formatter."""
    lib = abi.load_rtmi()
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    ny, nx = rgb8.shape[:2]
    need = lib.rtmi_ppm_p3(nx, ny, rgb8.ctypes.data, None, 0)
    buf = C.create_string_buffer(need)
    n = lib.rtmi_ppm_p3(nx, ny, rgb8.ctypes.data, buf, need)
    return buf.raw[:n]


def _denoise_params(iterations=5, normal_power=128, sigma_l=4.0, sigma_z=1.0, eps_l=1e-10, eps_z=1e-3, albedo_min=1e-3):
    """denoise()'s keywords as rtmi_denoise_params."""
    return abi.DenoiseParams(iterations, normal_power, sigma_l, sigma_z, eps_l, eps_z, albedo_min, 0)


def _temporal_params(max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3, demodulate=True):
    """Temporal's keywords as rtmi_temporal_params."""
    return abi.TemporalParams(max_history, alpha_min, depth_tol, normal_min, albedo_min,
                              0 if demodulate else abi.RTMI_TEMPORAL_NO_DEMODULATE)


def denoise(linear, albedo, normal, depth, stderr=None, iterations=5, normal_power=128, sigma_l=4.0, sigma_z=1.0,
            eps_l=1e-10, eps_z=1e-3, albedo_min=1e-3, device=0):
    """The a-trous denoiser of include/rtmi_denoise.h on `device`: linear, albedo, normal (and stderr, or None) are float32
    [ny,nx,3], depth is float32 [ny,nx] (non-finite = no surface), row 0 the top row.  Returns dict(linear f32 [ny,nx,3],
    rgb8 u8 [ny,nx,3]).  ValueError for a shape or dtype mismatch, HostError for what rtmi_denoise refuses."""
    depth = np.asarray(depth)
    if depth.ndim != 2:
        raise ValueError("depth must be [ny, nx], not %r" % (depth.shape,))
    ny, nx = depth.shape
    planes = _feature_planes(ny, nx, linear, albedo, normal, depth, stderr)
    p = _denoise_params(iterations, normal_power, sigma_l, sigma_z, eps_l, eps_z, albedo_min)
    lin = np.zeros((ny, nx, 3), np.float32)
    rgb = np.zeros((ny, nx, 3), np.uint8)
    lib = abi.load_rtmi()
    rc = lib.rtmi_denoise(device, nx, ny, C.byref(p), planes["linear"].ctypes.data, planes["albedo"].ctypes.data,
                          planes["normal"].ctypes.data, planes["depth"].ctypes.data,
                          planes["stderr"].ctypes.data if stderr is not None else None, lin.ctypes.data, rgb.ctypes.data)
    _rtmi_check(lib, rc, "rtmi_denoise")
    return {"linear": lin, "rgb8": rgb}


_denoise = denoise

_temporals = []  # the open Temporal handles; Host.free_all() closes them


class Temporal(_Handle):
    """The device-resident temporal history of include/rtmi_temporal.h for nx x ny images on `device`: push() reprojects
    the frames pushed so far into the new frame's camera and blends them with it.  demodulate=False sets
    RTMI_TEMPORAL_NO_DEMODULATE.  close() frees its device memory (184 B per pixel); Host.free_all() closes what is
    still open.  Usable as a context manager.  HostError for what rtmi_temporal_create refuses."""
    _closed = "temporal history"

    def __init__(self, nx, ny, device=0, max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3,
                 demodulate=True):
        self.lib = abi.load_rtmi()
        self.nx, self.ny, self.device = int(nx), int(ny), device
        p = _temporal_params(max_history, alpha_min, depth_tol, normal_min, albedo_min, demodulate)
        h = C.c_void_p()
        self._check(self.lib.rtmi_temporal_create(device, self.nx, self.ny, C.byref(p), C.byref(h)), "rtmi_temporal_create")
        self._opened(h, _temporals)

    def _destroy(self, h):
        self.lib.rtmi_temporal_destroy(h)

    def push(self, cam, linear, albedo, normal, depth, stderr=None, motion=False):
        """One frame: cam is the camera it was rendered with (a Camera of Host or an abi.Camera); linear, albedo, normal
        (and stderr, or None) are float32 [ny,nx,3], depth is float32 [ny,nx] (non-finite = no surface), row 0 the top row.
        Returns dict(linear f32 [ny,nx,3], stderr f32 [ny,nx,3] or None, history f32 [ny,nx][, motion f32 [ny,nx,2]]):
        linear and stderr are what denoise() takes.  ValueError for a shape or dtype mismatch, HostError for what
        rtmi_temporal_push refuses (a stderr given on some pushes and not on others, a singular camera)."""
        h = self._handle()
        c = cam.lower() if hasattr(cam, "lower") else cam
        ny, nx = self.ny, self.nx
        planes = _feature_planes(ny, nx, linear, albedo, normal, depth, stderr)
        out = {"linear": np.zeros((ny, nx, 3), np.float32),
               "stderr": np.zeros((ny, nx, 3), np.float32) if stderr is not None else None,
               "history": np.zeros((ny, nx), np.float32)}
        if motion:
            out["motion"] = np.zeros((ny, nx, 2), np.float32)
        rc = self.lib.rtmi_temporal_push(h, C.byref(c), planes["linear"].ctypes.data, planes["albedo"].ctypes.data,
                                         planes["normal"].ctypes.data, planes["depth"].ctypes.data,
                                         planes["stderr"].ctypes.data if stderr is not None else None,
                                         out["linear"].ctypes.data,
                                         out["stderr"].ctypes.data if stderr is not None else None,
                                         out["history"].ctypes.data, out["motion"].ctypes.data if motion else None)
        self._check(rc, "rtmi_temporal_push")
        return out

    def reset(self):
        """Forgets the frames pushed so far; the next push is a first push."""
        self._check(self.lib.rtmi_temporal_reset(self._handle()), "rtmi_temporal_reset")


_tonemaps = []  # the open Tonemap handles; Host.free_all() closes them


def _tonemap_params(op="aces", oetf="srgb", exposure="auto", ev=0.0, white=float("inf"), key=0.18, log2_range=(-12, 12),
                    percentiles=(0.10, 0.95), speed=(3.0, 1.0), adapt_range=None):
    """Tonemap's keywords as rtmi_tonemap_params."""
    for what, table, v in (("op", abi.TONEMAP_OPS, op), ("oetf", abi.TONEMAP_OETFS, oetf),
                           ("exposure", abi.TONEMAP_EXPOSURES, exposure)):
        if v not in table:
            raise ValueError("%s must be one of %s, not %r" % (what, ", ".join(sorted(table)), v))
    lo, hi = adapt_range if adapt_range is not None else log2_range
    return abi.TonemapParams(abi.TONEMAP_OPS[op], abi.TONEMAP_OETFS[oetf], abi.TONEMAP_EXPOSURES[exposure], 0, ev, white, key,
                             log2_range[0], log2_range[1], percentiles[0], percentiles[1], speed[0], speed[1], lo, hi, 0)


def _tonemap_state(st):
    return {"exposure": st.exposure, "adapted_log2": st.adapted_log2, "metered_log2": st.metered_log2,
            "counted": int(st.counted), "kept": int(st.kept), "applies": int(st.applies)}


class Tonemap(_Handle):
    """The tone mapper of include/rtmi_tonemap.h for nx x ny images on `device`: apply() meters the image's
    log-luminance histogram, adapts the exposure over the applies (exposure="auto"; "manual": 2^ev), applies the curve
    `op` ("clamp", "reinhard" with the white point `white`, "aces") and the transfer function `oetf` ("gamma2": the
    reference's sqrt quantiser; "srgb").  log2_range: the histogram's range, percentiles: the shares of the samples the
    mean leaves out below and keeps up to, speed: the adaptation's rates (up, down) per second, adapt_range: the bounds of
    the adapted value (None: log2_range).  close() frees its device memory; Host.free_all() closes what is still open.
    Usable as a context manager.  ValueError for an unknown name, HostError for what rtmi_tonemap_create refuses."""
    _closed = "tone mapper"

    def __init__(self, nx, ny, device=0, op="aces", oetf="srgb", exposure="auto", ev=0.0, white=float("inf"), key=0.18,
                 log2_range=(-12, 12), percentiles=(0.10, 0.95), speed=(3.0, 1.0), adapt_range=None):
        self.lib = abi.load_rtmi()
        self.nx, self.ny, self.device = int(nx), int(ny), device
        p = _tonemap_params(op, oetf, exposure, ev, white, key, log2_range, percentiles, speed, adapt_range)
        h = C.c_void_p()
        self._check(self.lib.rtmi_tonemap_create(device, self.nx, self.ny, C.byref(p), C.byref(h)), "rtmi_tonemap_create")
        self._opened(h, _tonemaps)

    def _destroy(self, h):
        self.lib.rtmi_tonemap_destroy(h)

    def apply(self, linear, dt=0.0, display=False, sync=None):
        """One image: linear is float32 [ny,nx,3], row 0 the top row; dt the seconds since the previous apply.
        A numpy array goes through the blocking host form and returns dict(rgb8 u8 [ny,nx,3][, display f32 [ny,nx,3]],
        exposure = dict(exposure, adapted_log2, metered_log2, counted, kept, applies)).  A torch tensor on the handle's device
        goes through the device form on torch's current stream, without a copy or a wait: it returns tensors, with state =
        the 32 bytes of rtmi_tonemap_state as a uint8 tensor, and the decoded exposure dict only with sync=True (which
        waits for the stream).  ValueError for a shape, dtype, device or contiguity mismatch, HostError for what the entry
        refuses (a misaligned tensor among it)."""
        h = self._handle()
        want = (self.ny, self.nx, 3)
        if isinstance(linear, np.ndarray) or not hasattr(linear, "data_ptr"):
            a = np.asarray(linear)
            _check_plane("linear", a, want)
            a = np.ascontiguousarray(a)
            out = {"rgb8": np.zeros(want, np.uint8)}
            if display:
                out["display"] = np.zeros(want, np.float32)
            st = abi.TonemapState()
            self._check(self.lib.rtmi_tonemap_apply(h, a.ctypes.data, dt, out["rgb8"].ctypes.data,
                                                    out["display"].ctypes.data if display else None, C.byref(st)),
                        "rtmi_tonemap_apply")
            out["exposure"] = _tonemap_state(st)
            return out
        import torch

        _check_plane("linear", linear, want, torch.float32)
        if not linear.is_cuda or linear.device.index != self.device:
            raise ValueError("linear must be on the handle's device (cuda:%d), not %s" % (self.device, linear.device))
        if not linear.is_contiguous():
            raise ValueError("linear must be contiguous")
        dev = linear.device
        out = {"rgb8": torch.empty(want, dtype=torch.uint8, device=dev)}
        if display:
            out["display"] = torch.empty(want, dtype=torch.float32, device=dev)
        out["state"] = torch.empty(32, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        self._check(self.lib.rtmi_tonemap_apply_device(h, linear.data_ptr(), dt, out["rgb8"].data_ptr(),
                                                       out["display"].data_ptr() if display else None,
                                                       out["state"].data_ptr(), stream.cuda_stream),
                    "rtmi_tonemap_apply_device")
        if sync:
            stream.synchronize()
            out["exposure"] = _tonemap_state(abi.TonemapState.from_buffer_copy(out["state"].cpu().numpy().tobytes()))
        return out

    def reset(self):
        """The next apply is a first apply: it adopts the metered value instead of adapting toward it."""
        self._check(self.lib.rtmi_tonemap_reset(self._handle()), "rtmi_tonemap_reset")


def tonemap(linear, device=0, display=False, **kw):
    """One image through a Tonemap made for it (create, apply once, close): linear float32 [ny,nx,3]; kw: Tonemap's
    keywords.  A first apply adopts the metered value, so exposure="auto" exposes the image for itself.  Returns
    Tonemap.apply's dict."""
    a = np.asarray(linear)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("linear must be [ny, nx, 3], not %r" % (a.shape,))
    with Tonemap(a.shape[1], a.shape[0], device=device, **kw) as tm:
        return tm.apply(a, display=display)


def _upscale_params(normal_power=32, sigma_z=0.05, eps_z=1e-3, albedo_min=1e-3, w_min=1e-3):
    """upscale()'s parameter keywords as rtmi_upscale_params."""
    return abi.UpscaleParams(normal_power, sigma_z, eps_z, albedo_min, w_min, 0)


def upscale(linear_lo, albedo_lo, normal_lo, depth_lo, albedo, normal, depth, device=0, **params):
    """The guided reconstruction of include/rtmi_upscale.h: linear_lo, albedo_lo and normal_lo are float32
    [ly,lx,3] and depth_lo float32 [ly,lx], the low-resolution image and its first-hit features; albedo, normal [ny,nx,3]
    and depth [ny,nx] are the full-resolution guide (non-finite depth = no surface), lx <= nx and ly <= ny, row 0 the top
    row.  params: normal_power=32, sigma_z=0.05, eps_z=1e-3, albedo_min=1e-3, w_min=1e-3.  numpy arrays go through the
    blocking host form on `device`; torch tensors (all on one device, contiguous) go through the device form on torch's
    current stream, without a copy or a wait.  Returns dict(linear f32 [ny,nx,3], rgb8 u8 [ny,nx,3], cls u8 [ny,nx]: 0
    background, 1 guided, 2 nearest-similar, 3 mismatch).  ValueError for a shape, dtype, device or contiguity mismatch,
    HostError for what the entry refuses (a misaligned tensor among it)."""
    names = ("linear_lo", "albedo_lo", "normal_lo", "depth_lo", "albedo", "normal", "depth")
    planes = dict(zip(names, (linear_lo, albedo_lo, normal_lo, depth_lo, albedo, normal, depth)))
    on_device = all(hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) for a in planes.values())
    if not on_device:
        planes = {n: np.asarray(a) for n, a in planes.items()}
    if planes["depth_lo"].ndim != 2 or planes["depth"].ndim != 2:
        raise ValueError("depth_lo and depth must be [ly, lx] and [ny, nx]")
    (ly, lx), (ny, nx) = tuple(planes["depth_lo"].shape), tuple(planes["depth"].shape)
    if on_device:
        import torch

        f32, dev = torch.float32, planes["depth"].device
    else:
        f32 = np.float32
    for n, a in planes.items():
        want = ((ly, lx) if n.endswith("_lo") else (ny, nx)) + (() if n.startswith("depth") else (3,))
        _check_plane(n, a, want, f32)
        if on_device:
            if not a.is_cuda or a.device != dev:
                raise ValueError("%s must be on the device of depth (%s), not %s" % (n, dev, a.device))
            if not a.is_contiguous():
                raise ValueError("%s must be contiguous" % n)
        else:
            planes[n] = np.ascontiguousarray(a)
    p = _upscale_params(**params)
    lib = abi.load_rtmi()
    if on_device:
        out = {"linear": torch.empty((ny, nx, 3), dtype=f32, device=dev), "rgb8": torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev),
               "cls": torch.empty((ny, nx), dtype=torch.uint8, device=dev)}
        i = abi.UpscaleIn(*[planes[n].data_ptr() for n in names])
        o = abi.UpscaleOut(out["linear"].data_ptr(), out["rgb8"].data_ptr(), out["cls"].data_ptr())
        rc, what = lib.rtmi_upscale_device(dev.index, lx, ly, nx, ny, C.byref(p), C.byref(i), C.byref(o),
                                           torch.cuda.current_stream(dev).cuda_stream), "rtmi_upscale_device"
    else:
        out = {"linear": np.zeros((ny, nx, 3), np.float32), "rgb8": np.zeros((ny, nx, 3), np.uint8), "cls": np.zeros((ny, nx), np.uint8)}
        i = abi.UpscaleIn(*[planes[n].ctypes.data for n in names])
        o = abi.UpscaleOut(out["linear"].ctypes.data, out["rgb8"].ctypes.data, out["cls"].ctypes.data)
        rc, what = lib.rtmi_upscale(device, lx, ly, nx, ny, C.byref(p), C.byref(i), C.byref(o)), "rtmi_upscale"
    _rtmi_check(lib, rc, what)
    return out


def _sparse_mask(classes):
    """The accept mask of a set of classes: bit c for every class c in 0..31."""
    mask = 0
    for c in classes:
        if not 0 <= int(c) < 32:
            raise ValueError("a class must be in 0..31, not %r" % (c,))
        mask |= 1 << int(c)
    return mask


def _sparse_device_of(t, device):
    if t.device.type != "cuda":
        raise ValueError("the tensor is on %s, not on a GPU" % (t.device,))
    return t.device.index if t.device.index is not None else device


def sparse_select(bytes, classes, capacity=None, device=0):
    """The ascending list of the pixels of a byte plane whose byte is in `classes` (rtmi_sparse_select_device of
    include/rtmi_sparse.h): bytes of 32 and above are never selected.  capacity: the most indices to write (None: the
    plane's size), the first in index order.  A torch uint8 tensor on a GPU is read in place and the call enqueued on
    torch's current stream: returns (list int32 [capacity] (the words of a uint32 list; those past counts[0] are not
    written), counts int32 [2] = (written, selected)) on that device, nothing is read back.  A numpy array goes through
    `device` and comes back as (list uint32 [written], counts uint32 [2])."""
    import torch

    mask = _sparse_mask(classes)
    torch_in = hasattr(bytes, "data_ptr") and hasattr(bytes, "is_cuda")
    if torch_in:
        if bytes.dtype != torch.uint8 or not bytes.is_contiguous():
            raise ValueError("bytes must be a contiguous uint8 tensor")
        b = bytes
        device = _sparse_device_of(b, device)
    else:
        a = np.ascontiguousarray(bytes)
        if a.dtype != np.uint8:
            raise ValueError("bytes must be a uint8 array")
        b = torch.from_numpy(a.reshape(-1)).to(torch.device("cuda", device))
    n = b.numel()
    cap = n if capacity is None else int(capacity)
    lib = abi.load_rtmi()
    dev = b.device
    lst = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    nbytes = int(lib.rtmi_sparse_scratch_bytes(n, 0, 0))
    scratch = torch.empty(((nbytes + 15) // 16, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtmi_sparse_select_device(device, n, C.c_void_p(b.data_ptr()), mask, cap, C.c_void_p(lst.data_ptr()),
                                           C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise HostError((lib.rtmi_last_error() or b"").decode())
    if torch_in:
        return lst[:cap], counts
    c = counts.cpu().numpy().view(np.uint32)
    return lst[:int(c[0])].cpu().numpy().view(np.uint32), c


def sparse_patch(pixels, mean, linear=None, rgb8=None, bytes=None, mark=4, count=None, device=0):
    """Writes records back where they belong (rtmi_sparse_patch_device of include/rtmi_sparse.h), in place, on torch's
    current stream: for each entry k of the int32 tensor `pixels` (of the first min(count[0], len) with a count tensor)
    whose pixel p lies inside the planes, linear[p] = mean[k], rgb8[p] = its quantised value, bytes[p] = mark.  All are
    contiguous torch tensors on one GPU: mean f32 [n, 3], linear f32 [..., 3], rgb8 u8 [..., 3], bytes u8 [...]; each plane
    is optional, the planes' pixel count comes from the first one given."""
    import torch

    planes = [(linear, 3), (rgb8, 3), (bytes, 1)]
    first = next(((a, ch) for a, ch in planes if a is not None), None)
    if first is None:
        raise ValueError("give at least one plane")
    n_pixels = first[0].numel() // first[1]
    for a, ch in planes:
        if a is not None and (a.numel() != n_pixels * ch or not a.is_contiguous()):
            raise ValueError("the planes must be contiguous and of one size")
    if pixels.dtype != torch.int32 or mean.dtype != torch.float32 or not pixels.is_contiguous() or not mean.is_contiguous():
        raise ValueError("pixels is a contiguous int32 tensor, mean a contiguous float32 tensor")
    dev = pixels.device
    device = _sparse_device_of(pixels, device)
    lib = abi.load_rtmi()
    ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    with torch.cuda.device(dev):
        rc = lib.rtmi_sparse_patch_device(device, n_pixels, ptr(pixels), ptr(count), pixels.numel(), ptr(mean), ptr(linear), ptr(rgb8),
                                          ptr(bytes), int(mark), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise HostError((lib.rtmi_last_error() or b"").decode())


def pfm_bytes(plane):
    """A float32 plane as PFM, the float format denoiser tools read: [ny,nx,3] -> "PF" (colour), [ny,nx] -> "Pf"
    (greyscale).  The scale is -1 (little-endian samples) and rows run bottom to top, so row 0 of the array (the top row,
    as every output here) is written last."""
    a = np.asarray(plane)
    if a.ndim == 3 and a.shape[2] == 3:
        tag = b"PF"
    elif a.ndim == 2:
        tag = b"Pf"
    else:
        raise ValueError("pfm_bytes takes an [ny,nx,3] or [ny,nx] array, not %r" % (a.shape,))
    ny, nx = a.shape[:2]
    body = np.ascontiguousarray(a[::-1], dtype="<f4").tobytes()
    return tag + b"\n%d %d\n-1.0\n" % (nx, ny) + body


def read_pfm(data):
    """The inverse of pfm_bytes: PFM bytes ("PF" colour or "Pf" greyscale, either byte order) -> float32 [ny,nx,3] or
    [ny,nx], row 0 the top row.  Loads HDR environment maps (Scene.attach_env)."""
    parts, pos = [], 0
    while len(parts) < 4:  # tag, width, height, scale: whitespace-separated tokens, then one whitespace byte
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        if end == pos:
            raise ValueError("read_pfm: truncated header")
        parts.append(data[pos:end])
        pos = end
    pos += 1
    tag, nx, ny, scale = parts[0], int(parts[1]), int(parts[2]), float(parts[3])
    if tag not in (b"PF", b"Pf") or nx <= 0 or ny <= 0 or scale == 0:
        raise ValueError("read_pfm: not a PFM header: %r" % (parts,))
    ch = 3 if tag == b"PF" else 1
    dt = np.dtype("<f4" if scale < 0 else ">f4")
    n = nx * ny * ch
    if len(data) - pos < 4 * n:
        raise ValueError("read_pfm: %d samples expected, %d bytes left" % (n, len(data) - pos))
    a = np.frombuffer(data, dtype=dt, count=n, offset=pos).astype(np.float32)
    a = a.reshape((ny, nx, 3) if ch == 3 else (ny, nx))[::-1]
    return np.ascontiguousarray(a)


def env_tables(rgb):
    """The sampling tables of an environment map (rtmi_env_tables, include/rtmi_env.h): float32 [H, W, 3] -> dict(row_cdf
    [H], row_p [H], col_cdf [H, W], col_p [H, W], total).  Host code: needs no GPU."""
    a = np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.float32:
        raise ValueError("env_tables takes a float32 [H, W, 3] array, not %s %r" % (a.dtype, a.shape))
    a = np.ascontiguousarray(a)
    h, w = a.shape[:2]
    lib = abi.load_rtmi()
    out = {"row_cdf": np.zeros(h, np.float32), "row_p": np.zeros(h, np.float32), "col_cdf": np.zeros((h, w), np.float32),
           "col_p": np.zeros((h, w), np.float32)}
    total = C.c_double(0.0)
    m = abi.EnvMap(w, h, a.ctypes.data)
    rc = lib.rtmi_env_tables(C.byref(m), out["row_cdf"].ctypes.data, out["row_p"].ctypes.data, out["col_cdf"].ctypes.data,
                             out["col_p"].ctypes.data, C.byref(total))
    if rc != 0:
        raise HostError("rtmi_env_tables failed (%d): %s" % (rc, lib.rtmi_last_error().decode()))
    out["total"] = total.value
    return out


def env_from_sky(width, height):
    """RTMI_FLAG_SKY's gradient as an environment map: float32 [height, width, 3], each texel the sky (f64, rounded once)
    in the direction of its centre."""
    j = np.arange(height, dtype=np.float64)
    theta = (1.0 - (j + 0.5) / height) * np.pi - np.pi / 2
    t = 0.5 * (np.sin(theta) + 1.0)
    a = 1.0 - t
    row = np.stack([a + t * 0.5, a + t * 0.7, a + t * 1.0], axis=-1)
    return np.ascontiguousarray(np.broadcast_to(row[:, None, :], (height, width, 3)).astype(np.float32))


def write_ppm(path, rgb8, fmt=3):
    """Stream the image to `path` without building the whole-image string: fmt 3 = the P3 text of create_image
    (byte-identical to ppm_p3), fmt 6 = binary P6."""
    lib = abi.load_rtmi()
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    ny, nx = rgb8.shape[:2]
    rc = lib.rtmi_write_ppm(os.fsencode(path), nx, ny, rgb8.ctypes.data, int(fmt))
    if rc != 0:
        raise HostError("rtmi_write_ppm failed (%d): %s" % (rc, lib.rtmi_last_error().decode()))
