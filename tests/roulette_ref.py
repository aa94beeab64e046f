"""Host-side restatement of Russian-roulette path termination (include/rtmi_roulette.h) for the plain estimator, from the
unchanged oracle.  numpy only; no GPU.

Under the plain estimator a sample's radiance is T_k * Le: the throughput after its k scatters times the emitter's value,
or 0 when the path never ends on an emitter.  In a scene whose scattering surfaces are all Lambertian with one SOLID
albedo `a` and whose emitters share one SOLID `Le`, T_j is the fp32 chain T_0 = 1, T_j = T_{j-1} * a whatever the
geometry, so the oracle's per-sample radiances give every lit sample's k by lookup in that chain.  From k, a, Le, the
Philox stream 4 and the header's pseudo-code the roulette radiance and scatter count of every sample follow; in a closed
scene an unlit path makes exactly max_depth scatters, so there every sample's count is known as well."""
import numpy as np

from nee_oracle_ref import welford_stderr  # noqa: F401  (re-exported for the tests)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox_word0(c0, c1, c2, c3, seed):
    """Word 0 of Philox4x32-10 for arrays of counters (broadcast), key = seed; vectorised philox.philox4x32_10."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & _MASK for c in (c0, c1, c2, c3)])
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _SH) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0.astype(np.uint32)


def roulette_u(depth, sample, pixel, seed):
    """u01 of the stream-4 word of the test at `depth` of path (sample, pixel), as float32."""
    w = philox_word0(depth, sample, pixel, 4, seed)
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def chain(albedo, n):
    """T_0 .. T_n [n + 1, 3] in fp32: T_0 = 1, T_j = T_{j-1} * a."""
    a = np.asarray(albedo, np.float32)
    t = np.ones((n + 1, 3), np.float32)
    for j in range(1, n + 1):
        t[j] = t[j - 1] * a
    return t


def lookup_k(samples, albedo, le, max_depth):
    """k [ny, nx, ns] of every sample of oracle.render_samples: the scatters before its emitter hit, -1 for a sample
    with radiance 0.  Asserts the condition of the whole method: no sample left out, i.e. every non-zero sample equals
    exactly one row of the chain times Le, and the rows are distinct."""
    t = chain(albedo, max_depth)
    rows = (t * np.asarray(le, np.float32)).astype(np.float32)
    assert np.all(np.isfinite(rows)) and np.all(np.abs(t[-1]) >= np.finfo(np.float32).tiny), "the chain leaves the normal floats"
    assert len({r.tobytes() for r in rows}) == len(rows), "chain rows are not distinct"
    hit = np.all(samples[..., None, :].view(np.uint32) == rows.view(np.uint32), axis=-1)  # [ny, nx, ns, max_depth + 1]
    lit = np.any(samples != 0, axis=-1)
    n = hit.sum(-1)
    assert np.all(n[lit] == 1), "%d lit samples match no chain row or several" % int(np.sum(n[lit] != 1))
    return np.where(lit, hit.argmax(-1), -1).astype(np.int64)


def restate(k, albedo, le, max_depth, min_depth, q_min, seed, nx, closed):
    """The roulette samples of rtmi_render_roulette's plain estimator: (samples f32 [ny, nx, ns, 3], scatters i64
    [ny, nx, ns], floor_survivals).  k: lookup_k's.  An unlit path runs to max_depth scatters in a closed scene; in an open
    one its length is unknown (it may leave the world) and its radiance is 0 either way, so open scenes return
    scatters = None.  floor_survivals counts the tests of LIT paths (their lengths are known in every scene) in which the
    floor was the binding term, m < q_min so q = q_min, and the path survived: T was divided by q_min itself."""
    ny, nx_, ns = k.shape
    assert nx_ == nx
    a = np.asarray(albedo, np.float32)
    le = np.asarray(le, np.float32)
    q_min = np.float32(q_min)
    row = np.arange(ny)[:, None, None]
    pixel = ((ny - 1 - row) * nx + np.arange(nx)[None, :, None]) + np.zeros((1, 1, ns), np.int64)
    sample = np.zeros((ny, nx, 1), np.int64) + np.arange(ns)[None, None, :]
    limit = np.where(k >= 0, k, max_depth)  # the scatters the path makes without roulette (unlit + closed: max_depth)
    T = np.ones((ny, nx, ns, 3), np.float32)
    alive = np.ones((ny, nx, ns), bool)
    scat = np.zeros((ny, nx, ns), np.int64)
    floor_survivals = 0
    for d in range(1, max_depth + 1):
        going = alive & (limit >= d)  # the path scatters a d-th time
        if not going.any():
            break
        T = np.where(going[..., None], (T * a).astype(np.float32), T)
        scat = np.where(going, d, scat)
        if d < min_depth:
            continue
        m = np.maximum(np.maximum(T[..., 0], T[..., 1]), T[..., 2])
        q = np.minimum(np.maximum(m, q_min), np.float32(1.0)).astype(np.float32)
        u = roulette_u(d, sample, pixel, seed)
        dead = going & ((m == 0) | ((q < 1) & ~(u < q)))
        resc = going & ~dead & (q < 1)
        floor_survivals += int(np.sum(resc & (k >= 0) & (m < q_min)))
        with np.errstate(divide="ignore", invalid="ignore"):
            T = np.where(resc[..., None], (T / q[..., None]).astype(np.float32), T)
        alive &= ~dead
    lit = alive & (k >= 0)
    out = np.where(lit[..., None], (T * le).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return out, (scat if closed else None), floor_survivals


def image(samples):
    """render's outputs of per-sample radiances [ny, nx, ns, 3]: the f64 sum in sample order / ns -> (linear f32, rgb8 u8)."""
    ns = samples.shape[2]
    col = np.zeros(samples.shape[:2] + (3,), np.float64)
    for s in range(ns):
        col = col + samples[:, :, s, :].astype(np.float64)
    m = col / float(ns)
    g = np.sqrt(m)
    g = np.where(g > 0.0, np.where(g < 1.0, g, 1.0), 0.0)
    return m.astype(np.float32), (255.99 * g).astype(np.int32).astype(np.uint8)


# ---- the uniform-albedo scenes (backend-agnostic: host or oracle `api`) -----------------------------------------------------
LE = (12.0, 12.0, 12.0)
BOXES = {  # name: (albedo, closed, max_depth)
    "open": ((0.5, 0.5, 0.5), False, 50),
    "closed": ((0.73, 0.73, 0.73), True, 50),
    "coloured": ((0.65, 0.45, 0.12), True, 24),  # 0.12^24 ~ 8e-23 stays a normal float; ^50 would not
}


def box(api, name, nx, ny):
    """A Cornell-style box of rects with a sphere and a cube inside and one ceiling lamp, every scatterer Lambertian with
    the one SOLID albedo of BOXES[name], every normal turned inward.  closed: a front wall behind the camera and an outer
    shell around the box, so no path leaves the world."""
    albedo, closed, _ = BOXES[name]
    mat = api.Lambertian(api.SolidTexture(*albedo))
    lamp = api.DiffuseLight(api.SolidTexture(*LE))
    w = api.HittableList()

    def shell(lo, hi):
        w.push(api.Rect(api.PLANE_YZ, lo, lo, hi, hi, lo, mat))
        w.push(api.FlipNormals(api.Rect(api.PLANE_YZ, lo, lo, hi, hi, hi, mat)))
        w.push(api.Rect(api.PLANE_ZX, lo, lo, hi, hi, lo, mat))
        w.push(api.FlipNormals(api.Rect(api.PLANE_ZX, lo, lo, hi, hi, hi, mat)))
        w.push(api.FlipNormals(api.Rect(api.PLANE_XY, lo, lo, hi, hi, hi, mat)))
        if closed:
            w.push(api.Rect(api.PLANE_XY, lo, lo, hi, hi, lo, mat))

    shell(0.0, 10.0)
    if closed:
        shell(-5.0, 15.0)
    w.push(api.Rect(api.PLANE_ZX, 3.5, 3.5, 6.5, 6.5, 9.9, lamp))
    w.push(api.Sphere((3.0, 1.5, 6.0), 1.5, mat))
    w.push(api.Cube((5.5, 0.0, 2.5), (8.0, 3.0, 5.0), mat))
    z0 = 0.5 if closed else -14.0
    cam = api.Camera((5.0, 5.0, z0), (5.0, 5.0, 10.0), (0.0, 1.0, 0.0), 80.0 if closed else 40.0, nx / ny, 0.0, 10.0, 0.0, 1.0)
    return cam, w
