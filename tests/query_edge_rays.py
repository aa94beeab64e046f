"""Edge rays for the ray queries (tests/test_query_edge_rays.py checks the corpus itself, tests/test_gpu_query_edges.py runs
it on the device): the rays a caller sends and a renderer never produces — axis-aligned, with one component exactly +-0,
starting on a surface, lying in a primitive's or a node box's plane, scaled by powers of two, with t_min at and around a
hit, and touching a sphere exactly.  Per scene `corpus` returns named families, each a dict of o, d (float32 [n, 3]),
times ([n] or None), t_min, t_max (float32 [n]), ref (the fp32 oracle's records, query_ref.oracle_records) and cls.

cls is decided from the ray, the scene description and the oracle alone:
  B: every ray of `in_plane` (o_k equal to a plane constant of the scene, d_k = +-0 or a denormal whose reciprocal
     overflows: 0 * inf = NaN in rect.rs and in aabb.rs), and any ray whose oracle record has a NaN in t or p (a hit accepted with t = NaN that nothing overwrote);
  A: everything else.  Class A rays equal the oracle bit for bit on the device.
Seeds are fixed; nothing here needs a GPU."""
import itertools

import numpy as np

import query_ref as Q
import test_media_in_bvh as media_worlds
SCENES = ["cornell_box", "random_spheres", "final_scene", "media_in_bvh", "sphere_lattice", "cube_lattice"]
FAMILIES = ["axis", "planar", "on_surface", "in_plane", "scaled", "interval", "grazing"]
LATTICES = ["sphere_lattice", "cube_lattice"]
FLAT = ["cornell_box", "cube_lattice_flat"]  # the top level and every member are plain lists
EXPONENTS = (-70, -40, 40, 62, 66)
LIGHT_K = 554.0  # final_scene's light: Rect(ZX, 147, 412, 123, 423, k = 554), x0 > x1, left out by the lowering
F32 = np.float32


# ---- the two hand-built worlds -------------------------------------------------------------------------------------------
def sphere_lattice(api, seed=1):
    """4x4x4 touching spheres of radius 1 at the even integer centres 0..6 and one MovingSphere of radius 0.5 in the gap
    around (3, 3, 3), all in one BVHNode: every node plane of the static spheres is an odd integer, where no static
    sphere is hit (the planes are tangent) but the moving sphere is."""
    api.seed_scene_rng(seed)
    mats = [api.Lambertian(api.SolidTexture(0.7, 0.3, 0.2)), api.Metal(api.SolidTexture(0.8, 0.8, 0.9), 0.1), api.Dielectric(1.5)]
    objs = [api.Sphere((2.0 * i, 2.0 * j, 2.0 * k), 1.0, mats[(i + j + k) % 3])
            for i, j, k in itertools.product(range(4), repeat=3)]
    objs.append(api.MovingSphere((3.0, 3.0, 3.0), (3.0, 3.125, 3.0), 0.0, 1.0, 0.5, api.DiffuseLight(api.SolidTexture(4.0, 4.0, 4.0))))
    return api.BVHNode(objs, 0.0, 1.0)


def cube_lattice(api, seed=1, flat=False, objects=False):
    """3x3x3 unit cubes [2i, 2i + 1]^3 with unit gaps, the middle one inside Traslate(RotateY(30)), in one BVHNode; flat:
    the same objects in a plain HittableList; objects: the list of the 27 objects itself, cube (i, j, k) at 9i + 3j + k."""
    api.seed_scene_rng(seed)
    mats = [api.Lambertian(api.SolidTexture(0.2, 0.6, 0.3)), api.Metal(api.SolidTexture(0.7, 0.6, 0.5), 0.0)]
    objs = []
    for i, j, k in itertools.product(range(3), repeat=3):
        m = mats[(i + j + k) % 2]
        if (i, j, k) == (1, 1, 1):
            objs.append(api.Traslate(api.Rotate(api.AXIS_Y, api.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), 30.0), (2.0, 2.0, 2.0)))
        else:
            objs.append(api.Cube((2.0 * i, 2.0 * j, 2.0 * k), (2.0 * i + 1.0, 2.0 * j + 1.0, 2.0 * k + 1.0), m))
    if objects:
        return objs
    if not flat:
        return api.BVHNode(objs, 0.0, 1.0)
    world = api.HittableList()
    for ob in objs:
        world.push(ob)
    return world


class WithoutNeverHitRects:
    """An api whose Rect with x0 > x1 or y0 > y1 is dropped from the lists it is pushed to: the world the lowering keeps
    (rt_host.cpp never_hit).  The reference accepts an in-plane ray on such a rect; the device cannot."""

    def __init__(self, api):
        self._api = api

    def __getattr__(self, name):
        return getattr(self._api, name)

    def Rect(self, plane, x0, y0, x1, y1, k, material):
        return None if x0 > x1 or y0 > y1 else self._api.Rect(plane, x0, y0, x1, y1, k, material)

    def HittableList(self):
        lst = self._api.HittableList()
        push = lst.push
        lst.push = lambda h: None if h is None else push(h)
        return lst


# the fans' cameras of the lattices, the box of the part of every scene that the origins are drawn around, the scenes with a time per ray
_LAT_CAMS = {"sphere_lattice": ((3.3, 3.7, -9.1), (3.0, 3.0, 3.0)), "cube_lattice": ((2.3, 2.9, -7.2), (2.5, 2.5, 2.5))}
_BOX = {"cornell_box": ((0.0, 0.0, 0.0), (555.0, 555.0, 555.0)), "random_spheres": ((-11.0, 0.0, -11.0), (11.0, 2.0, 11.0)),
        "final_scene": ((-200.0, 0.0, -200.0), (600.0, 560.0, 600.0)), "media_in_bvh": ((-6.0, -1.0, -3.0), (5.0, 3.5, 5.0)),
        "sphere_lattice": ((-1.0, -1.0, -1.0), (7.0, 7.0, 7.0)), "cube_lattice": ((0.0, 0.0, 0.0), (5.0, 5.0, 5.0))}
_TIMED = {"random_spheres", "media_in_bvh", "sphere_lattice"}


def build_world(api, name):
    if name == "media_in_bvh":
        return media_worlds.world_media_in_bvh(api)
    if name == "sphere_lattice":
        return sphere_lattice(api)
    if name in ("cube_lattice", "cube_lattice_flat"):
        return cube_lattice(api, flat=name.endswith("_flat"))
    return Q.build_world(api, name)


def camera(name):
    if name == "media_in_bvh":
        return (1.0, 3.0, 9.0), (0.0, 0.6, 0.5)
    if name.startswith("cube_lattice"):
        return _LAT_CAMS["cube_lattice"]
    return _LAT_CAMS[name] if name in _LAT_CAMS else Q.scene_camera(name)


def valid(s):
    """rtmi_validate_rays' rule (include/rtmi_query.h): finite components (t_max may be +inf), d != 0, t_min <= t_max"""
    ok = np.isfinite(s["o"]).all(axis=1) & np.isfinite(s["d"]).all(axis=1) & (s["d"] != 0).any(axis=1)
    ok &= np.isfinite(s["t_min"]) & ~np.isnan(s["t_max"]) & (s["t_max"] > -np.inf) & (s["t_min"] <= s["t_max"])
    return ok if s["times"] is None else ok & np.isfinite(s["times"])


# ---- plane constants of a lowered scene -----------------------------------------------------------------------------------
def _tree_prims(a, root):
    out, todo = [], [root]
    while todo:
        n = a["nodes"][todo.pop()]
        for ch in (n.left, n.right):
            if ch >= 0:
                todo.append(ch)
            else:
                out.append(ch & 0x0FFFFFFF)
    return out


def _tree_nodes(a, root):
    out, todo = [], [root]
    while todo:
        i = todo.pop()
        out.append(i)
        n = a["nodes"][i]
        todo += [ch for ch in (n.left, n.right) if ch >= 0]
    return out


def _frame_offset(a, first, count):
    """the y offset of a chain of Traslate / RotateY records, or None when the chain holds anything else: under such a
    chain the y planes of the object's frame are y planes of the world, moved by the offset"""
    off = F32(0.0)
    for x in a["xforms"][first:first + count]:
        if x.kind == 0:
            off = F32(off + F32(x.y))
        elif x.kind != 2:
            return None
    return off


def planes(a):
    """(axis, constant, lo[3], hi[3], what) of every rect, cube face and BVH node box plane of the lowered scene `a`
    (LoweredScene.arrays()) that is a plane of the world's frame: all three axes for an object without transforms, the y
    planes under Traslate / RotateY.  lo, hi: the extent of the primitive or the box in that frame."""
    out = []

    def box_planes(mn, mx, off, axes, what):
        mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
        if max(np.abs(mn).max(), np.abs(mx).max()) > 1e30:  # the box of a tree that holds media: +-FLT_MAX
            return
        for k in axes:
            for c in (mn[k], mx[k]):
                lo, hi = mn.copy(), mx.copy()
                lo[1], hi[1] = lo[1] + off, hi[1] + off
                out.append((k, F32(c + off) if k == 1 else F32(c), lo, hi, what))

    for it in a["items"]:
        if it.flags & 128:  # the terminator of a list scan holds no geometry
            continue
        off = _frame_offset(a, it.xform_first, it.xform_count)
        if off is None:
            continue
        axes = (0, 1, 2) if it.xform_count == 0 else (1,)
        prims = _tree_prims(a, it.first) if it.kind == 1 else range(it.first, it.first + it.count)
        if it.kind == 1:
            box_planes(it.root_min, it.root_max, off, axes, "node")
            for i in _tree_nodes(a, it.first):
                n = a["nodes"][i]
                box_planes(n.lmin, n.lmax, off, axes, "node")
                box_planes(n.rmin, n.rmax, off, axes, "node")
        for p in prims:
            m, A, B = a["prim_meta"][p], a["prim_a"][p], a["prim_b"][p]
            pax, poff = axes, off
            cnt = (m.flags >> 4) & 15
            if cnt:  # an instanced primitive's own chain
                po = _frame_offset(a, m.flags >> 12, cnt)
                if po is None:
                    continue
                pax, poff = (1,), F32(off + po)
            if m.type == 2:
                k = (m.flags >> 8) & 3
                ka, aa, ba = {0: (0, 1, 2), 1: (1, 2, 0), 2: (2, 0, 1)}[k]  # rect.rs:40-44
                if ka in pax:
                    lo, hi = np.zeros(3, F32), np.zeros(3, F32)
                    lo[ka] = hi[ka] = B[0]
                    lo[aa], lo[ba], hi[aa], hi[ba] = A[0], A[1], A[2], A[3]
                    box_planes(lo, hi, poff, (ka,), "rect")
            elif m.type == 3:
                box_planes((A[0], A[1], A[2]), (A[3], B[0], B[1]), poff, pax, "cube")
    return out


def in_face_plane(a, o, d):
    """bool [n]: ray i lies in the plane of a rect or a cube face of the lowered scene `a` (o_k equal to its constant,
    1 / d_k infinite: d_k = +-0 or a denormal up to 2^-128): Rect::hit computes t = 0 * inf = NaN there and accepts,
    wherever the ray is in that plane (rect.rs:46-51)"""
    out = np.zeros(o.shape[0], bool)
    inf = inv_d_infinite(d)
    for k, c, _, _, what in planes(a):
        if what != "node":
            out |= (o[:, k] == c) & inf[:, k]
    return out


def inv_d_infinite(d):
    """bool [n, 3]: 1 / d_k overflows in fp32 (aabb.rs:33 on the device): d_k = +-0, or denormal with |d_k| <= 2^-128"""
    with np.errstate(all="ignore"):
        return np.isinf(F32(1.0) / np.asarray(d, F32))


def node_boxes(a):
    """[m, 2, 3] float32: the boxes of every BVH item of `a` in the world's frame (items without transforms): the root
    boxes and both child boxes of every node"""
    out = []
    for it in a["items"]:
        if it.kind != 1 or it.xform_count or (it.flags & 128):
            continue
        out.append((list(it.root_min), list(it.root_max)))
        for i in _tree_nodes(a, it.first):
            n = a["nodes"][i]
            out += [(list(n.lmin), list(n.lmax)), (list(n.rmin), list(n.rmax))]
    return np.asarray(out, F32).reshape(-1, 2, 3)


def nan_slab(o, d, boxes):
    """bool [n]: AABB::hit (aabb.rs:33-36) of ray i meets a NaN slab value, (plane - o_k) * (1 / d_k) = 0 * inf, at some box"""
    bad = np.zeros(o.shape[0], bool)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / d
        for k in range(3):
            for side in (0, 1):
                bad |= np.isnan((boxes[None, :, side, k] - o[:, None, k]) * inv[:, None, k]).any(axis=1)
    return bad


# ---- the families -----------------------------------------------------------------------------------------------------------
def _uniform(rng, lo, hi, n, grow=0.0):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    g = grow * (hi - lo)
    return rng.uniform(lo - g, hi + g, (n, 3)).astype(F32)


def _signed_zero(negative):
    return F32(-0.0) if negative else F32(0.0)


def _axis_dirs():
    """the six axis directions, their two zero components in all four sign combinations of +-0: [24, 3]"""
    out = []
    for k in range(3):
        for s in (1.0, -1.0):
            for za, zb in itertools.product((False, True), repeat=2):
                d = np.zeros(3, F32)
                d[k], d[(k + 1) % 3], d[(k + 2) % 3] = s, _signed_zero(za), _signed_zero(zb)
                out.append(d)
    return np.array(out, F32)


def _axis(name, rng):
    lo, hi = _BOX[name]
    org = [_uniform(rng, lo, hi, 16, grow=0.3)]  # outside and inside, generic coordinates
    if name == "sphere_lattice":
        # on the node planes: integer origins, and generic origins with one odd integer coordinate (0 * inf at every
        # node whose box ends there; no static sphere is hit from there, the moving sphere is)
        org.append(rng.integers(-2, 9, (12, 3)).astype(F32))
        mixed = _uniform(rng, (2.6, 2.6, 2.6), (3.4, 3.6, 3.4), 12)
        for i in range(12):
            mixed[i, i % 3] = F32(rng.choice([1.0, 3.0, 3.0, 5.0]))
            mixed[i, (i + 1 + i // 3 % 2) % 3] -= F32(rng.choice([0.0, 6.0]))  # half of them start outside the lattice
        org.append(mixed)
    org = np.concatenate(org)
    dirs = _axis_dirs()
    return np.repeat(org, len(dirs), axis=0), np.tile(dirs, (len(org), 1))


def _planar(name, rng, n=384):
    lo, hi = _BOX[name]
    o = _uniform(rng, lo, hi, n, grow=0.4)
    d = (_uniform(rng, lo, hi, n).astype(np.float64) - o).astype(F32)
    for i in range(n):
        d[i, i % 3] = _signed_zero((i // 3) % 2 == 1)
    return o, d


def _times(name, rng, n):
    return rng.uniform(0.0, 1.0, n).astype(F32) if name in _TIMED else None


def _family(orc, world, o, d, times, t_min=Q.T_MIN, t_max=Q.INF, in_plane=False):
    n = o.shape[0]
    s = {"o": np.ascontiguousarray(o, F32), "d": np.ascontiguousarray(d, F32), "times": times,
         "t_min": np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, F32), (n,))),
         "t_max": np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, F32), (n,)))}
    s["ref"] = Q.oracle_records(orc, world, s["o"], s["d"], times, s["t_min"], s["t_max"])
    nan = np.isnan(s["ref"]["t"]) | np.isnan(s["ref"]["p"]).any(axis=1)
    s["cls"] = np.where(nan | in_plane, "B", "A")
    for c in "AB":  # the rays of either class as a set of its own: the device traces one class at a time
        s[c] = subset(orc, world, s, np.flatnonzero(s["cls"] == c))
    return s


def subset(orc, world, s, idx):
    """rays idx of the set s with the oracle's records of their own: ray j of the subset is traced with the seed
    query_ref.SEED + j, as the device draws for ray j of a call"""
    if len(idx) == len(s["cls"]):
        return s
    sub = {k: (None if s[k] is None else np.ascontiguousarray(s[k][idx])) for k in ("o", "d", "times", "t_min", "t_max")}
    sub["ref"] = Q.oracle_records(orc, world, sub["o"], sub["d"], sub["times"], sub["t_min"], sub["t_max"])
    sub["index"] = idx
    return sub


def _in_plane(name, a, rng, cap=1008):
    """rays in the planes of `a`: per plane an origin inside the primitive's (or box's) extent, one next to it and one
    outside the scene, each with a random direction in the plane and with an axis direction; d_k is +-0, +-1e-40 or
    +-2^-130 in turn: 1 / d_k is infinite for all of them, and the denormal ones have no zero component"""
    lo_s, hi_s = (np.asarray(v, np.float64) for v in _BOX[name])
    cand = planes(a)
    if name == "final_scene":  # the rect that the lowering drops is in no array: from the description
        cand.append((1, F32(LIGHT_K), np.array([123.0, LIGHT_K, 147.0], F32), np.array([423.0, LIGHT_K, 412.0], F32), "dropped"))
    seen, uniq = set(), []
    for c in cand:  # one entry per (axis, constant, kind); rects and the dropped rect first, then cubes, then nodes
        key = (c[0], float(c[1]), c[4])
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    order = {"dropped": 0, "rect": 1, "cube": 2, "node": 3}
    uniq.sort(key=lambda c: order[c[4]])
    first = [c for c in uniq if c[4] in ("dropped", "rect")]
    rest = [c for c in uniq if c[4] not in ("dropped", "rect")]
    per = 12
    first = first * 6 if len(first) * 6 * per <= cap // 4 else first  # several rays of each kind in the few rect planes
    room = max(cap // per - len(first), 0)
    if len(rest) > room:
        rest = [rest[i] for i in sorted(rng.choice(len(rest), room, replace=False))]
    chosen = first + rest
    chosen = chosen * max(1, min(4, cap // (per * len(chosen))))  # few planes: several rays of each kind per plane
    o, d, dropped = [], [], []
    for k, c, lo, hi, what in chosen:
        lo, hi = lo.astype(np.float64), hi.astype(np.float64)
        size = np.maximum(hi - lo, 1e-3 * (hi_s - lo_s))
        for place in range(3):
            for axial in (False, True):
                for neg in (False, True):
                    if place == 0:
                        p = rng.uniform(lo, np.maximum(hi, lo))
                    elif place == 1:
                        p = rng.uniform(lo, np.maximum(hi, lo)) + size * rng.choice([-1.5, 1.5], 3)
                    else:
                        p = hi_s + (hi_s - lo_s) * rng.uniform(0.1, 0.5, 3)
                    p = p.astype(F32)
                    p[k] = c
                    v = rng.standard_normal(3).astype(F32)
                    if axial:
                        j = (k + 1 + int(rng.integers(2))) % 3
                        v[:] = _signed_zero(rng.integers(2) == 1)
                        v[j] = F32(1.0) if place == 2 or rng.integers(2) else F32(-1.0)
                        if place == 2:  # from outside the scene: towards it
                            v[j] = F32(-1.0)
                    v[k] = F32((0.0, 1e-40, 2.0 ** -130)[len(o) % 3]) * F32(-1.0 if neg else 1.0)
                    o.append(p)
                    d.append(v)
                    dropped.append(what == "dropped")
    return np.array(o, F32), np.array(d, F32), np.array(dropped, bool)


def _grazing(name):
    """sphere_lattice: axis rays at distance exactly r from a sphere's centre line (b^2 - a c = 0 exactly, and in the
    device's form a (r^2 - |l|^2) = 0 exactly as well), and the same rays with the touching coordinate of the origin one
    ulp nearer and one ulp farther.  cube_lattice: diagonal rays through a point of a cube's edge, where two faces are
    hit at one t, and their neighbours 2^-10 to either side.  Returns o, d, times, tangent (bool: the exact ones), centre [n, 3], radius [n]."""
    o, d, tm, exact, cen, rad = [], [], [], [], [], []
    if name == "sphere_lattice":
        spheres = [((2.0 * i, 2.0 * j, 2.0 * k), 1.0, 0.0) for i, j, k in ((0, 0, 0), (3, 3, 3), (1, 2, 0), (2, 1, 3))]
        spheres += [((3.0, 3.0, 3.0), 0.5, 0.0), ((3.0, 3.125, 3.0), 0.5, 1.0)]  # the moving sphere at both ends of the shutter
        for c, r, time in spheres:
            for k in range(3):  # the ray's axis
                for j in ((k + 1) % 3, (k + 2) % 3):  # the axis of the offset
                    for side in (1.0, -1.0):
                        for step in (0, 1, -1):
                            for speed in (1.0, -2.0, 0.5):
                                p = np.array(c, F32)
                                p[j] = F32(c[j] + side * r)
                                if step:
                                    p[j] = np.nextafter(p[j], F32(np.inf if step > 0 else -np.inf))
                                p[k] = F32(c[k] - 4.0 * np.sign(speed))
                                v = np.zeros(3, F32)
                                v[k] = speed
                                o.append(p); d.append(v); tm.append(time); exact.append(step == 0); cen.append(c); rad.append(r)
    else:
        for base in ((2.0, 0.0, 0.0), (4.0, 2.0, 4.0), (0.0, 4.0, 2.0)):  # the corner (x0, y0, z0) of an axis-aligned cube
            for y in (0.5, 0.75, 0.25):
                for step in (0, 1, -1):
                    for dz in (1.0, 2.0, -1.0, -0.5):  # dz < 0: the ray only touches the edge and leaves the cube behind
                        p = np.array([base[0] - 1.0, base[1] + y, base[2] - dz], F32)  # through the edge x = x0, z = z0
                        p[0] += F32(step * 2.0 ** -10)  # (every product stays exact in fp32: the neighbours miss or hit for good)
                        o.append(p); d.append(np.array([1.0, 0.0 if y != 0.25 else 0.125, dz], F32)); tm.append(0.0)
                        exact.append(False); cen.append(base); rad.append(0.0)
    return (np.array(o, F32), np.array(d, F32), np.array(tm, F32), np.array(exact, bool), np.array(cen, np.float64),
            np.array(rad, np.float64))


def cube_lattice_leaf_fold(orc, a, s):
    """What the device returns for the rays s on cube_lattice's tree, restated from its rule (include/rtmi_query.h): a leaf
    is reached when the boxes of all its ancestors pass AABB::hit with the query's own interval, as in the reference; the
    leaves that accept are folded in sequence, left to right — a later leaf replaces the best so far unless best.t < t,
    which a NaN on either side fails — where BVHNode::hit folds the two results of every node (bvh.rs:75-81).  Boxes and
    tree from the lowered arrays, box tests and leaf records from the oracle's probes (the 27 objects one by one).
    Returns (prim [n], -1 for a miss; records like query_ref.oracle_records)."""
    objs = cube_lattice(orc, objects=True)
    of_prim = []  # the object of every lowered primitive
    for m, A in zip(a["prim_meta"], a["prim_a"]):
        i, j, k = (1, 1, 1) if (m.flags >> 4) & 15 else (int(A[0]) // 2, int(A[1]) // 2, int(A[2]) // 2)
        of_prim.append(9 * i + 3 * j + k)
    assert sorted(of_prim) == list(range(27))
    n = len(s["ref"]["hit"])
    o64, d64 = s["o"].astype(np.float64), s["d"].astype(np.float64)
    t_max = np.where(np.isinf(s["t_max"]), 1.8e308, s["t_max"].astype(np.float64))

    def box(mn, mx, mask):
        out = mask.copy()
        for i in np.flatnonzero(mask):
            out[i] = orc.aabb_hit(o64[i], d64[i], list(mn) + list(mx), float(s["t_min"][i]), float(t_max[i]), flags=Q.ARITH_DEVICE)
        return out

    (item,) = a["items"]
    leaves = []  # (primitive, rays that reach it), left to right

    def walk(node, mask):
        nd = a["nodes"][node]
        for side, (child, mn, mx) in enumerate(((nd.left, nd.lmin, nd.lmax), (nd.right, nd.rmin, nd.rmax))):
            if side == 1 and nd.right == nd.left:  # a BVHNode over one object: the same leaf twice, same result
                continue
            if child < 0:  # a leaf child has no box test of its own (bvh.rs:72-73)
                leaves.append((child & 0x0FFFFFFF, mask))
            else:
                walk(child, box(mn, mx, mask))

    walk(item.first, box(item.root_min, item.root_max, np.ones(n, bool)))
    assert sorted(p for p, _ in leaves) == list(range(27))
    per = {p: Q.oracle_records(orc, objs[of_prim[p]], s["o"], s["d"], s["times"], s["t_min"], s["t_max"]) for p, _ in leaves}
    prim = np.full(n, -1)
    best_t = np.zeros(n, F32)
    for p, mask in leaves:
        r = per[p]
        with np.errstate(invalid="ignore"):
            take = mask & r["hit"] & ((prim < 0) | ~(best_t < r["t"]))
        prim[take], best_t[take] = p, r["t"][take]
    rec = Q.oracle_records(orc, objs[0], s["o"][:0], s["d"][:0])  # the miss record's fields
    rec = {k: np.concatenate([v, np.zeros((n,) + v.shape[1:], v.dtype)]) for k, v in rec.items()}
    rec["t"][:], rec["mat_kind"][:] = np.inf, -1
    for p, _ in leaves:
        for k in rec:
            rec[k][prim == p] = per[p][k][prim == p]
    return prim, rec


_CACHE = {}


def corpus(orc, host, name):
    """The families of a scene, built once: dict(family -> dict(o, d, times, t_min, t_max, ref, cls)).  orc: the fp32
    oracle; host: the host mirror, for the lowered arrays the planes are read from.  `in_plane` of final_scene also has
    `dropped` (bool: the ray lies in the plane of the rect the lowering leaves out) and `ref_lowered`, the oracle's
    records of the world without that rect; `grazing` has `tangent`, `centre` and `radius`."""
    if name in _CACHE:
        return _CACHE[name]
    flat = name.endswith("_flat")
    base = name[:-5] if flat else name
    world = build_world(orc, name)
    a = host.lower(build_world(host, name)).arrays()
    # the records are views into the lowered scene, which the host frees when a test ends: keep copies
    a = {k: [type(x).from_buffer_copy(x) for x in v] if isinstance(v, list) else v for k, v in a.items()}
    seeds = np.random.SeedSequence(20240 + SCENES.index(base)).spawn(8)
    rngs = [np.random.default_rng(s) for s in seeds]
    out = {}
    timed = base in _TIMED

    o, d = _axis(base, rngs[0])
    out["axis"] = _family(orc, world, o, d, _times(base, rngs[0], len(o)))
    o, d = _planar(base, rngs[1])
    out["planar"] = _family(orc, world, o, d, _times(base, rngs[1], len(o)))

    look_from, look_at = camera(name)
    fo, fd = Q.fan(rngs[2], look_from, look_at, 256)
    ft = _times(base, rngs[2], 256)
    fan = Q.oracle_records(orc, world, fo, fd, ft)
    hits = np.flatnonzero(fan["hit"] & ~np.isnan(fan["p"]).any(axis=1))

    # on_surface: from the fan's hit points, each with t_min = 0 and 0.001
    so = np.repeat(fan["p"][hits], 2, axis=0)
    sd = np.repeat(rngs[3].standard_normal((len(hits), 3)).astype(F32), 2, axis=0)
    st = None if not timed else np.repeat(ft[hits], 2)
    out["on_surface"] = _family(orc, world, so, sd, st, t_min=np.tile(np.array([0.0, Q.T_MIN], F32), len(hits)))

    o, d, dropped = _in_plane(base, a, rngs[4])
    out["in_plane"] = _family(orc, world, o, d, _times(base, rngs[4], len(o)), in_plane=True)
    if base == "final_scene":
        s = out["in_plane"]
        s["dropped"] = dropped
        s["ref_lowered"] = Q.oracle_records(orc, build_world(WithoutNeverHitRects(orc), name), s["o"], s["d"], s["times"],
                                            s["t_min"], s["t_max"])

    # scaled: d * 2^e (t scales by 2^-e), and o and d both * 2^20
    k = 128
    o = np.concatenate([fo[:k]] * len(EXPONENTS) + [fo[:k] * F32(2.0 ** 20)])
    d = np.concatenate([fd[:k] * F32(2.0 ** e) for e in EXPONENTS] + [fd[:k] * F32(2.0 ** 20)])
    out["scaled"] = _family(orc, world, o, d, None if not timed else np.tile(ft[:k], len(EXPONENTS) + 1))

    # interval: t_min at the hit, one ulp to either side, -t and -1e30; and t_min == t_max == t
    h = hits[:150]
    t = fan["t"][h]
    up, down = np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))
    tmins = [t, up, down, -t, np.full(len(h), -1e30, F32), t]
    tmaxs = [np.full(len(h), np.inf, F32)] * 5 + [t]
    out["interval"] = _family(orc, world, np.tile(fo[h], (6, 1)), np.tile(fd[h], (6, 1)), None if not timed else np.tile(ft[h], 6),
                              t_min=np.concatenate(tmins), t_max=np.concatenate(tmaxs))

    if base in LATTICES:
        o, d, tm, exact, cen, rad = _grazing(base)
        s = _family(orc, world, o, d, tm if timed else None)
        s["tangent"], s["centre"], s["radius"] = exact, cen, rad
        out["grazing"] = s
    for s in out.values():
        s["meets_nan"] = in_face_plane(a, s["o"], s["d"])
    orc.free_all()
    out["arrays"] = a
    _CACHE[name] = out
    return out


def families(c):
    """the ray families of a corpus (without its `arrays` entry)"""
    return {k: v for k, v in c.items() if k != "arrays"}


def counts(c):
    """per family: rays, hits, class B"""
    return {k: (len(s["cls"]), int(s["ref"]["hit"].sum()), int((s["cls"] == "B").sum())) for k, s in families(c).items()}
