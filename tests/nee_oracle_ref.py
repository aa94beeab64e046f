"""Host-side restatements for the oracle tests of next-event estimation (include/rtmi_nee.h, include/rtmi_adaptive.h):
the light table in the device's order with its selection probabilities, and the standard error of the mean by
Welford's recurrence.  numpy only; no GPU."""
import numpy as np

from oracle.oracle import KIND_RECT, LIGHT_DTYPE

RTMI_PRIMFLAG_PLANE_SHIFT = 8


def device_geometry(sc):
    """(kind, plane, geo[5]) of every light of the lowered scene's table (rtmi_lights_from_desc), in table order, read
    from the flat description the way rtmi_scene_attach_lights does."""
    t = sc.lights()
    a = sc.arrays()
    out = []
    for L in t:
        A, B = a["prim_a"][L["prim"]], a["prim_b"][L["prim"]]
        if L["kind"] == KIND_RECT:
            plane = (a["prim_meta"][L["prim"]].flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3
            geo = (A[0], A[1], A[2], A[3], B[0])
        else:
            plane, geo = -1, (A[0], A[1], A[2], A[3], 0.0)
        out.append((int(L["kind"]), int(plane), np.array(geo, np.float64)))
    return t, out


def match_emitters(emitters, dev_geo):
    """Indices into `emitters` (Oracle.emitters) of the device's lights, one to one, by kind, plane and geometry.
    Raises AssertionError when a device light has no eligible oracle emitter or an eligible emitter is left over."""
    free = {}
    for i in range(len(emitters)):
        if emitters["eligible"][i]:
            key = (int(emitters["kind"][i]), int(emitters["plane"][i]), tuple(emitters["geo"][i].tolist()))
            free.setdefault(key, []).append(i)
    idx = []
    for kind, plane, geo in dev_geo:
        key = (kind, plane, tuple(geo.tolist()))
        assert free.get(key), "device light %s %s has no eligible oracle emitter" % (kind, geo)
        idx.append(free[key].pop(0))
    left = [i for v in free.values() for i in v]
    assert not left, "oracle emitters %s are eligible but not device lights" % [emitters["geo"][i].tolist() for i in left]
    return idx


def selection(area, weight):
    """p_sel = area * w / sum(area * w) and its CDF, in f64, as rtmi_nee.h specifies: the sum accumulated in table
    order, the running sum of p_sel in table order, the last entry exactly 1."""
    aw = [float(a) * float(w) for a, w in zip(area, weight)]
    total = 0.0
    for x in aw:
        total += x
    p = [x / total for x in aw]
    cdf, c = [], 0.0
    for i, x in enumerate(p):
        c += x
        cdf.append(1.0 if i + 1 == len(p) else c)
    return np.array(p, np.float64), np.array(cdf, np.float64)


def light_table(emitters, idx):
    """The oracle's light table (LIGHT_DTYPE) of emitters[idx] in that order: area, p_sel and cdf rounded to float as
    rtmi_scene_attach_lights rounds them."""
    e = emitters[list(idx)]
    p, cdf = selection(e["area"], e["weight"])
    t = np.zeros(len(e), LIGHT_DTYPE)
    t["handle"], t["kind"], t["plane"], t["geo"] = e["handle"], e["kind"], e["plane"], e["geo"]
    t["area"] = e["area"].astype(np.float32)
    t["p_sel"] = p.astype(np.float32)
    t["cdf"] = cdf.astype(np.float32)
    return t


def oracle_lights(orc, world, sc):
    """The oracle's light table of `world` (built on `orc`) in the order of the device's table of `sc` (the same scene
    lowered by the host)."""
    em = orc.emitters(world)
    _, geo = device_geometry(sc)
    return light_table(em, match_emitters(em, geo))


def welford_stderr(samples):
    """include/rtmi_adaptive.h's standard error of per-sample radiances [..., ns, 3] (fp32): widened to double, in
    sample order, d = x - m; m = m + d / k; M2 = M2 + d * (x - m); stderr = sqrt(M2 / (n (n - 1))), rounded to float.
    Vectorised over pixels, sequential over k; numpy evaluates each operation with one rounding (no fused operations)."""
    x = samples.astype(np.float64)
    n = x.shape[-2]
    m = np.zeros(x.shape[:-2] + (3,))
    M2 = np.zeros_like(m)
    for k in range(n):
        xk = x[..., k, :]
        d = xk - m
        m = m + d / float(k + 1)
        M2 = M2 + d * (xk - m)
    return np.sqrt(M2 / (float(n) * (float(n) - 1.0))).astype(np.float32)


# ---- hand-built scenes that make NEE's rarely taken branches happen (backend-agnostic: host or oracle `api`) -----------
def _cam(api, look_from, look_at, nx, ny, vfov=40.0):
    return api.Camera(look_from, look_at, (0.0, 1.0, 0.0), vfov, nx / ny, 0.0, 10.0, 0.0, 1.0)


def _lamb(api, a=0.7):
    return api.Lambertian(api.SolidTexture(a, a, a))


def _light(api, le):
    return api.DiffuseLight(api.SolidTexture(le, le, le))


def edge_inside_sphere_light(api, nx, ny):
    """Lambertian vertices inside a sphere light: no light sample toward it and p_l = 0 on its BSDF hits."""
    w = api.HittableList()
    w.push(api.Sphere((0.0, 0.0, 0.0), 10.0, _light(api, 0.5)))
    w.push(api.Sphere((0.0, 0.0, 0.0), 1.5, _lamb(api)))
    w.push(api.Rect(api.PLANE_ZX, -1.0, -1.0, 1.0, 1.0, 4.0, _light(api, 3.0)))
    return _cam(api, (0.0, 1.0, 6.0), (0.0, 0.0, 0.0), nx, ny, 50.0), w


def edge_tiny_far_sphere(api, nx, ny):
    """A sphere light of r = 0.01 about 10 away from the lit floor (s ~ 1e-6), next to an ordinary rect light."""
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, -20.0, -20.0, 20.0, 20.0, 0.0, _lamb(api)))
    w.push(api.Sphere((0.0, 10.0, 0.0), 0.01, _light(api, 2.0e5)))
    w.push(api.Rect(api.PLANE_XY, -2.0, 2.0, 2.0, 4.0, -6.0, _light(api, 2.0)))
    return _cam(api, (0.0, 2.0, 8.0), (0.0, 0.0, 0.0), nx, ny), w


def edge_grazing_rect(api, nx, ny):
    """Rect lights almost coplanar with the lit floor: a lamp 1e-3 above it and a wall lamp standing on it (cos_l -> 0,
    p_l toward FLT_MAX)."""
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, -20.0, -20.0, 20.0, 20.0, 0.0, _lamb(api)))
    w.push(api.Rect(api.PLANE_ZX, -3.0, -3.0, 3.0, 3.0, 0.001, _light(api, 4.0)))
    w.push(api.Rect(api.PLANE_YZ, 0.0, -4.0, 2.0, 4.0, 4.0, _light(api, 4.0)))
    return _cam(api, (-2.0, 3.0, 9.0), (1.0, 0.0, 0.0), nx, ny), w


def edge_light_in_medium(api, nx, ny):
    """A rect light inside a fog volume: every shadow ray's free flight draws from the light-sample stream."""
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, -20.0, -20.0, 20.0, 20.0, 0.0, _lamb(api)))
    w.push(api.Rect(api.PLANE_ZX, -1.0, -1.0, 1.0, 1.0, 2.5, _light(api, 6.0)))
    w.push(api.ConstantMedium(api.Cube((-4.0, 0.0, -4.0), (4.0, 4.0, 4.0), api.Dielectric(1.5)), 0.15,
                              api.SolidTexture(0.8, 0.8, 0.8)))
    return _cam(api, (0.0, 3.0, 10.0), (0.0, 1.0, 0.0), nx, ny), w


def edge_listscan_light(api, nx, ny):
    """A light that is a member of a list with media, itself a child of a BVHNode (a LISTSCAN group, rtmi.h)."""
    grp = api.HittableList()
    grp.push(api.ConstantMedium(api.Sphere((1.0, 1.0, 0.0), 1.0, api.Dielectric(1.5)), 0.8, api.SolidTexture(0.9, 0.9, 0.9)))
    grp.push(api.Sphere((-1.0, 2.5, 0.0), 0.6, _light(api, 5.0)))
    grp.push(api.Sphere((-1.5, 0.7, 1.0), 0.7, _lamb(api, 0.6)))
    objs = [grp, api.Sphere((0.0, -1000.0, 0.0), 1000.0, _lamb(api, 0.5)), api.Sphere((2.5, 0.5, 1.5), 0.5, _lamb(api, 0.8)),
            api.Sphere((0.0, 4.0, -2.0), 0.4, _light(api, 3.0))]
    return _cam(api, (0.0, 2.0, 9.0), (0.0, 1.0, 0.0), nx, ny), api.BVHNode(objs, 0.0, 1.0)


def edge_deferred_lights(api, nx, ny):
    """Lights among DEFERRED items: a BVHNode whose children are an instanced subtree and a medium next to two lights."""
    inner = api.BVHNode([api.Sphere((0.0, 0.5, 0.0), 0.5, _lamb(api, 0.6)), api.Cube((1.0, 0.0, 0.0), (2.0, 1.0, 1.0), _lamb(api)),
                         api.Sphere((-1.0, 0.4, 1.0), 0.4, _lamb(api, 0.9))], 0.0, 1.0)
    objs = [api.Traslate(api.Rotate(api.AXIS_Y, inner, 25.0), (0.5, 0.0, -0.5)),
            api.ConstantMedium(api.Sphere((-2.0, 1.0, 0.0), 1.0, api.Dielectric(1.5)), 0.5, api.SolidTexture(0.7, 0.8, 0.9)),
            api.Sphere((0.0, 3.0, 0.0), 0.5, _light(api, 6.0)),
            api.Rect(api.PLANE_XY, -1.0, 0.5, 1.0, 2.0, -3.0, _light(api, 3.0)),
            api.Rect(api.PLANE_ZX, -10.0, -10.0, 10.0, 10.0, 0.0, _lamb(api, 0.5))]
    return _cam(api, (1.0, 2.5, 8.0), (0.0, 0.8, 0.0), nx, ny), api.BVHNode(objs, 0.0, 1.0)


def edge_bvh_moving_occluders(api, nx, ny):
    """Sphere lights in a BVH of many spheres, moving Lambertian spheres among them as occluders (the shadow ray's
    time is the path's)."""
    import numpy as np

    rng = np.random.default_rng(11)
    objs = [api.Sphere((0.0, -1000.0, 0.0), 1000.0, _lamb(api, 0.5))]
    for k in range(40):
        c = (float(rng.uniform(-4, 4)), float(rng.uniform(0.3, 3.0)), float(rng.uniform(-4, 4)))
        r = float(rng.uniform(0.15, 0.4))
        if k % 8 == 0:
            objs.append(api.Sphere(c, r, _light(api, float(rng.uniform(2.0, 8.0)))))
        elif k % 3 == 0:
            objs.append(api.MovingSphere(c, (c[0], c[1] + 0.8, c[2]), 0.0, 1.0, r, _lamb(api, 0.8)))
        else:
            objs.append(api.Sphere(c, r, _lamb(api, float(rng.uniform(0.3, 0.9)))))
    return _cam(api, (0.0, 3.0, 11.0), (0.0, 1.0, 0.0), nx, ny, 45.0), api.BVHNode(objs, 0.0, 1.0)


def edge_cdf_extremes(api, nx, ny):
    """Two lights whose area x weight differ by 10^6: the small one first (cdf[0] ~ 1e-6), then the large one."""
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, -20.0, -20.0, 20.0, 20.0, 0.0, _lamb(api)))
    w.push(api.Rect(api.PLANE_ZX, 0.0, 0.0, 0.01, 0.01, 3.0, _light(api, 1.0)))
    w.push(api.Rect(api.PLANE_ZX, -5.0, -5.0, 5.0, 5.0, 4.0, _light(api, 1.0)))
    return _cam(api, (0.0, 2.0, 8.0), (0.0, 0.0, 0.0), nx, ny), w


def edge_isotropic_rect(api, nx, ny):
    """An Isotropic medium lit by a rect (p_b = 1 / (4 pi) at its vertices)."""
    w = api.HittableList()
    w.push(api.ConstantMedium(api.Sphere((0.0, 1.0, 0.0), 1.5, api.Dielectric(1.5)), 1.0, api.SolidTexture(0.9, 0.6, 0.3)))
    w.push(api.Rect(api.PLANE_XY, -2.0, 0.0, 2.0, 3.0, -3.0, _light(api, 5.0)))
    return _cam(api, (0.0, 1.0, 7.0), (0.0, 1.0, 0.0), nx, ny), w


def edge_cdf_boundaries(api, nx, ny):
    """4096 equal lamps (0.25 x 0.25, coordinates exact in fp32) in one tree facing a lit wall: p_sel = 2^-12 and every cdf
    entry k / 4096 exactly, so a 24-bit uniform equals an entry once in ~4100 light samples and the search's strict
    `us < cdf` decides which lamp it picks."""
    lamps = []  # XY rects: the only plane whose bounding box (rect.rs:71-75) is right, so they can sit in a tree
    for i in range(64):
        for k in range(64):
            x, y = -16.0 + 0.5 * i, -16.0 + 0.5 * k
            lamps.append(api.Rect(api.PLANE_XY, x, y, x + 0.25, y + 0.25, 3.0, _light(api, 2.0)))
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_XY, -30.0, -30.0, 30.0, 30.0, 0.0, _lamb(api, 0.6)))
    w.push(api.BVHNode(lamps, 0.0, 1.0))
    return api.Camera((0.0, 0.0, 1.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 90.0, nx / ny, 0.0, 1.0, 0.0, 1.0), w


EDGE = {f.__name__[5:]: f for f in (edge_inside_sphere_light, edge_tiny_far_sphere, edge_grazing_rect, edge_light_in_medium,
                                     edge_listscan_light, edge_deferred_lights, edge_bvh_moving_occluders, edge_cdf_extremes,
                                     edge_isotropic_rect, edge_cdf_boundaries)}
