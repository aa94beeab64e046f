"""Render sessions (include/rtmi_session.h) on the device.

Every equality is on the raw bits of every plane; the references are the one-shot entries, which sessions leave untouched,
the oracle's per-sample radiances, and the numpy restatement of tests/session_ref.py.

1. continue == one-shot for every estimator, with and without roulette, per-lane and cooperative, however N is split;
2. first_sample: a session that starts at sample 7 against the oracle's samples 7..15;
3. checkpoint: export, destroy, create, import, continue; damaged blobs are refused and change nothing;
4. refine == one-shot adaptive after every call of a tightening sequence, an off-lattice cap included; no sample twice;
5. merge == the numpy restatement bit for bit, and within 1 ulp / 1 level of the one-shot render;
6. hygiene: cancellation and the failed state, two sessions on one scene, stats, render_for."""
import numpy as np
import pytest

import env_ref
import scenes_extra
import session_ref as sr
from nee_oracle_ref import oracle_lights
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HostError, Unsupported

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
COOP, PERLANE = abi.RTMI_KERNEL_WAVE_COOP, abi.RTMI_KERNEL_PERLANE
RR = dict(min_depth=2, q_min=0.25)
PLANES = ("linear", "rgb8", "stderr")


def _build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=1)


def _scene(host, name, mapname, nx, ny):
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    if mapname:
        sc.attach_env(env_ref.sun_map())
    return cam, sc


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_planes(label, got, ref, planes):
    for key in planes:
        a, b = got[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key)
        bad = int(np.sum(_bits(a) != _bits(b)))
        assert bad == 0, "%s: %d of %d words of %s differ" % (label, bad, a.size, key)


def _one_shot(sc, cam, nx, ny, ns, est, rr, coop, adaptive=None, **kw):
    """The one-shot entry a session of (est, rr) equals: fixed with ns samples, or adaptive = (min_spp, step_spp, abs_tol)."""
    kw = {"seed": SEED, "flags": FC, **kw}
    if rr:
        if adaptive:
            return sc.render_adaptive_roulette(cam, nx, ny, ns, adaptive[0], adaptive[1], abs_tol=adaptive[2], estimator=est,
                                               env_select_p=0.5, coop=coop, **RR, **kw)
        return sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, coop=coop, **RR, **kw)
    if adaptive or est == "plain":
        a = adaptive or (ns, 1, 0.0)
        lit = est != "plain"
        return sc.render_adaptive(cam, nx, ny, ns, a[0], a[1], abs_tol=a[2], nee=est in ("nee", "env_nee"),
                                  env=est in ("env", "env_nee"), env_select_p=0.5, coop=coop and lit, **kw)
    if est == "nee":
        return sc.render_nee(cam, nx, ny, ns, coop=coop, **kw)
    return sc.render_env(cam, nx, ny, ns, nee=est == "env_nee", env_select_p=0.5, coop=coop, **kw)


def _session(sc, cam, nx, ny, est, rr, coop, **kw):
    kw = {"seed": SEED, "flags": FC, **kw}
    return sc.session(cam, nx, ny, estimator=est, roulette=RR if rr else None, env_select_p=0.5, coop=coop, **kw)


def _planes(rr, extra=()):
    return PLANES + tuple(extra) + (("bounces",) if rr else ())


# ---- 1. continue == one-shot -----------------------------------------------------------------------------------------------
CASES = [("cornell_box", None, "plain"), ("cornell_box", None, "nee"), ("lit_smoke", None, "nee"),
         ("random_spheres", "sun", "env"), ("random_spheres", "sun", "env_nee")]


@pytest.mark.gpu
@pytest.mark.parametrize("coop", [False, True], ids=["perlane", "coop"])
@pytest.mark.parametrize("rr", [False, True], ids=["rr0", "rr1"])
@pytest.mark.parametrize("name,mapname,est", CASES, ids=["%s-%s" % (n, e) for n, _, e in CASES])
def test_continue_equals_one_shot(host, name, mapname, est, rr, coop):
    nx, ny, N = 37, 21, 16  # ragged on both edges
    cam, sc = _scene(host, name, mapname, nx, ny)
    ref = _one_shot(sc, cam, nx, ny, N, est, rr, coop)
    three = ((nx + 7) // 8) * ((ny + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES * 3  # every call runs sub-passes
    for split in ((5, 1, 10), (2, 14)):
        ses = _session(sc, cam, nx, ny, est, rr, coop, sample_buffer_bytes=three)
        traced = 0
        for add in split:
            st = ses.render(add)
            assert st["samples"] == nx * ny * add and st["kernel"] == ref["stats"]["kernel"], (split, st)
            traced += add
            assert ses.spp() == (traced, traced)
        img = ses.image()
        _same_planes("%s %s rr%d coop%d %s" % (name, est, rr, coop, split), img, ref, _planes(rr))
        assert np.all(img["spp"] == N)
        if not rr:
            assert not img["bounces"].any()
        ses.close()
    if coop and name == "random_spheres":
        assert ref["stats"]["kernel"] == COOP
    if rr:
        assert ref["bounces"].any()
    if est == "plain" and not rr:  # FAST_CULL, SYNC and REF_TREE do not change the bits
        for flags in (0, FC | abi.RTMI_FLAG_SYNC, FC | abi.RTMI_FLAG_REF_TREE):
            ses = _session(sc, cam, nx, ny, est, rr, coop, flags=flags)
            ses.render(9)
            ses.render(7)
            _same_planes("flags %d" % flags, ses.image(), ref, PLANES)
            ses.close()


# ---- 2. first_sample -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("est", ["plain", "nee"])
def test_first_sample_against_the_oracle(host, orc32, est):
    nx, ny, s0, n = 24, 24, 7, 9
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    cam_o, world_o = _build(orc32, "cornell_box", nx, ny)
    if est == "plain":
        ref = orc32.render_samples(cam_o, world_o, nx, ny, s0 + n, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM)
    else:
        ref = orc32.render_nee(cam_o, world_o, oracle_lights(orc32, world_o, sc), nx, ny, s0 + n, seed=SEED,
                               flags=ARITH_DEVICE | THROUGHPUT_FORM, samples=True)
    orc32.free_all()
    x = ref["samples"][:, :, s0:s0 + n]
    s, _, M2 = (a[n] for a in sr.accumulate(x))
    lin, rgb = sr.quantise(s, n)
    want = {"linear": lin, "rgb8": rgb, "stderr": sr.stderr_of(M2, n).astype(np.float32)}
    ses = _session(sc, cam, nx, ny, est, False, False, first_sample=s0)
    ses.render(4)
    ses.render(5)
    _same_planes(est, ses.image(), want, PLANES)
    whole = _session(sc, cam, nx, ny, est, False, False)  # and the range is not the first nine samples
    whole.render(n)
    assert not np.array_equal(whole.image()["linear"], want["linear"])


# ---- 3. checkpoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_checkpoint_and_damaged_blobs(host):
    nx, ny = 37, 21
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    ref = _one_shot(sc, cam, nx, ny, 16, "nee", True, False)
    ses = _session(sc, cam, nx, ny, "nee", True, False)
    ses.render(6)
    blob = ses.save()
    b = sr.parse_blob(blob)
    assert (b["nx"], b["ny"], b["kind"], b["estimator"], b["rr"], b["seed"]) == (nx, ny, 0, 1, 1, SEED) and np.all(b["n"] == 6)
    _same_planes("parsed blob", sr.readout(b), ses.image(), _planes(True, ("spp",)))
    ses.close()
    with pytest.raises(HostError, match="closed"):
        ses.render(1)
    ses = _session(sc, cam, nx, ny, "nee", True, False)
    ses.load(blob)
    assert ses.spp() == (6, 6)
    ses.render(10)
    _same_planes("restored", ses.image(), ref, _planes(True))
    before = ses.image()
    bad_seed = bytearray(blob)
    bad_seed[sr.SEED_OFFSET] ^= 1
    other = _session(sc, cam, 24, 24, "nee", True, False)
    other.render(2)
    other_before = other.image()
    for label, target, data, what in (("seed", ses, bytes(bad_seed), "identity"), ("truncated", ses, blob[:-8], "length"),
                                      ("short", ses, blob[:100], "magic"), ("size", other, blob, "identity"),
                                      ("magic", ses, b"X" + blob[1:], "magic")):
        with pytest.raises(HostError, match=what):
            target.load(data)
    _same_planes("unchanged", ses.image(), before, _planes(True, ("spp",)))
    _same_planes("unchanged", other.image(), other_before, _planes(True, ("spp",)))
    assert ses.spp() == (16, 16) and other.spp() == (2, 2)


# ---- 4. refine == one-shot adaptive ----------------------------------------------------------------------------------------
def _tile_max(a, nx, ny):
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, 3), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, 3).max(axis=(1, 3, 4))


SEQUENCES = {"tighten": [(2.0, 24), (1.0, 24), (0.5, 48)], "off_lattice_cap": [(1.0, 20), (0.5, 48)]}
REFINE = [("plain", False, False), ("nee", False, False), ("nee", True, False), ("nee", False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("est,rr,coop", REFINE, ids=["%s-rr%d-coop%d" % c for c in REFINE])
def test_refine_equals_one_shot_adaptive(host, est, rr, coop, seq):
    nx, ny = 40, 24
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    first = _one_shot(sc, cam, nx, ny, 8, est, rr, coop, adaptive=(8, 8, 0.0))
    u = float(np.median(_tile_max(first["stderr"].astype(np.float64), nx, ny)))
    assert u > 0
    ses = _session(sc, cam, nx, ny, est, rr, coop, lattice=(8, 8))
    planes = _planes(rr, ("spp",))
    traced, history = 0, []
    for scale, cap in SEQUENCES[seq]:
        st = ses.refine(scale * u, 0.0, cap)
        traced += st["samples"]
        ref = _one_shot(sc, cam, nx, ny, cap, est, rr, coop, adaptive=(8, 8, scale * u))
        img = ses.image()
        counts = {int(k): int((img["spp"] == k).sum()) // 64 for k in np.unique(img["spp"])}
        print(est, rr, coop, seq, "tol %.2fu cap %d:" % (scale, cap), counts, "this call", st["samples"], "one-shot", ref["stats"]["samples"])
        _same_planes("%s tol %.2fu cap %d" % (seq, scale, cap), img, ref, planes)
        assert traced == ref["stats"]["samples"]  # no sample traced twice
        assert st["kernel"] == ref["stats"]["kernel"]
        again = ses.refine(scale * u, 0.0, cap)  # a repeated identical call traces nothing and changes nothing
        assert again["samples"] == 0
        _same_planes("repeat", ses.image(), img, planes)
        history.append(img["spp"].copy())
        if seq == "off_lattice_cap" and len(history) == 1:  # the rest of the sequence runs on a restored checkpoint
            blob = ses.save()
            assert sr.parse_blob(blob)["last_cap"] == cap and sr.parse_blob(blob)["kind"] == 1
            ses.close()
            ses = _session(sc, cam, nx, ny, est, rr, coop, lattice=(8, 8))
            ses.load(blob)
            _same_planes("restored", ses.image(), img, planes)
    # the conditions without which the test would pass vacuously
    assert len(np.unique(history[-1])) >= 3, np.unique(history[-1])
    assert np.any(history[0] < history[-1])  # a tile parked by the first call and advanced by a later one
    assert np.any(history[0] == history[-1])  # ... and one that stayed parked
    if seq == "off_lattice_cap":
        assert np.any(history[0] == 20)
    cap = SEQUENCES[seq][-1][1]
    for args in ((0.6 * u, 0.0, cap), (0.5 * u, 1e-6, cap), (0.5 * u, 0.0, cap - 1)):
        with pytest.raises(HostError, match="loosen"):
            ses.refine(*args)
    with pytest.raises(HostError, match="REFINE"):
        ses.render(4)
    _same_planes("after the refusals", ses.image(), img, planes)


@pytest.mark.gpu
def test_wrong_kind_of_call_and_bad_arguments(host):
    cam, sc = _scene(host, "cornell_box", None, 24, 24)
    fixed = _session(sc, cam, 24, 24, "nee", False, False)
    with pytest.raises(HostError, match="FIXED"):
        fixed.refine(0.1, 0.0, 16)
    with pytest.raises(HostError, match="add_spp"):
        fixed.render(0)
    with pytest.raises(HostError, match="no samples"):
        fixed.image()
    with pytest.raises(Unsupported, match="2\\^26"):
        fixed.render(1 << 27)
    with pytest.raises(HostError, match="2\\^31"):
        fixed.render((1 << 31) + 5)
    refine = _session(sc, cam, 24, 24, "nee", False, False, lattice=(8, 8))
    with pytest.raises(HostError, match="cap"):
        refine.refine(0.1, 0.0, 4)
    with pytest.raises(HostError, match="finite"):
        refine.refine(float("nan"), 0.0, 16)
    bare_cam, bare_world = _build(host, "cornell_box", 24, 24)
    bare = host.lower(bare_world).upload(0)
    with pytest.raises(HostError, match="env"):
        bare.session(bare_cam, 24, 24, estimator="env")


# ---- 5. merge --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("est,rr", [("nee", False), ("plain", True)], ids=["nee", "plain-rr"])
def test_merge(host, est, rr):
    nx, ny = 24, 24
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    a, b = _session(sc, cam, nx, ny, est, rr, False), _session(sc, cam, nx, ny, est, rr, False, first_sample=8)
    a.render(8)
    b.render(8)
    blob_a, blob_b, img_b = a.save(), b.save(), b.image()
    a.merge(b)
    assert a.spp() == (16, 16) and b.spp() == (8, 8)
    _same_planes("src unchanged", b.image(), img_b, _planes(rr, ("spp",)))
    got = a.image()
    want = sr.readout(sr.merge(sr.parse_blob(blob_a), sr.parse_blob(blob_b)))
    _same_planes("restatement", got, want, _planes(True, ("spp",)))
    merged_state = sr.parse_blob(a.save())
    assert np.array_equal(merged_state["state"], sr.merge(sr.parse_blob(blob_a), sr.parse_blob(blob_b))["state"])
    ref = _one_shot(sc, cam, nx, ny, 16, est, rr, False)
    d_lin = int(sr.ulps(got["linear"], ref["linear"]).max())
    d_se = int(sr.ulps(got["stderr"], ref["stderr"]).max())
    d_rgb = int(np.abs(got["rgb8"].astype(np.int32) - ref["rgb8"].astype(np.int32)).max())
    print("merge %s rr%d against the one-shot 16: linear %d ulp, stderr %d ulp, rgb8 %d levels" % (est, rr, d_lin, d_se, d_rgb))
    assert d_lin <= 1 and d_rgb <= 1
    if rr:
        assert np.array_equal(got["bounces"], ref["bounces"]) and ref["bounces"].any()
    # an empty dst copies, an empty src is a no-op
    empty, c = _session(sc, cam, nx, ny, est, rr, False), _session(sc, cam, nx, ny, est, rr, False)
    c.render(8)
    empty.merge(c)
    _same_planes("copy", empty.image(), c.image(), _planes(True, ("spp",)))
    tail = _session(sc, cam, nx, ny, est, rr, False, first_sample=16)
    a.merge(tail)
    _same_planes("no-op", a.image(), got, _planes(True, ("spp",)))
    # refusals: a gap, an overlap, unequal identity, a refine session
    gap, overlap = (_session(sc, cam, nx, ny, est, rr, False, first_sample=s) for s in (17, 15))
    other_seed = _session(sc, cam, nx, ny, est, rr, False, first_sample=16, seed=SEED + 1)
    refine = _session(sc, cam, nx, ny, est, rr, False, lattice=(8, 8))
    for s in (gap, overlap, other_seed):
        s.render(2)
    for src, what in ((gap, "adjacent"), (overlap, "adjacent"), (other_seed, "identity"), (refine, "REFINE"), (a, "one session")):
        with pytest.raises(HostError, match=what):
            a.merge(src)
    _same_planes("after the refusals", a.image(), got, _planes(True, ("spp",)))


# ---- 6. hygiene ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cancellation_leaves_the_session_failed_until_an_import(host):
    nx, ny = 37, 21
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    cancel = [False]
    seen = []

    def progress(done, total):
        seen.append((done, total))
        return cancel[0]

    ses = _session(sc, cam, nx, ny, "nee", False, False, progress=progress)
    ses.render(6)
    assert seen and seen[-1][0] == seen[-1][1] and all(d <= t for d, t in seen)
    blob, img = ses.save(), ses.image()
    cancel[0] = True
    with pytest.raises(HostError, match="cancelled"):
        ses.render(4)
    for call in (lambda: ses.render(4), ses.image, ses.save, ses.spp):
        with pytest.raises(HostError, match="failed"):
            call()
    cancel[0] = False
    ses.load(blob)
    _same_planes("restored", ses.image(), img, PLANES + ("spp",))
    ses.render(10)
    _same_planes("continued", ses.image(), _one_shot(sc, cam, nx, ny, 16, "nee", False, False), PLANES)


@pytest.mark.gpu
def test_two_sessions_on_one_scene_stats_and_render_for(host):
    nx, ny = 37, 21
    cam, sc = _scene(host, "cornell_box", None, nx, ny)
    cam2 = host.Camera((278.0, 278.0, -700.0), (200.0, 300.0, 0.0), (0.0, 1.0, 0.0), 40.0, nx / ny, 0.0, 10.0, 0.0, 1.0)
    a, b = _session(sc, cam, nx, ny, "nee", False, False), _session(sc, cam2, nx, ny, "plain", True, False)
    for add in (3, 5):  # interleaved, with one-shot renders of the scene in between
        a.render(add)
        sc.render_nee(cam2, nx, ny, 4, seed=SEED, flags=FC)
        b.render(add)
    _same_planes("a", a.image(), _one_shot(sc, cam, nx, ny, 8, "nee", False, False), PLANES)
    _same_planes("b", b.image(), _one_shot(sc, cam2, nx, ny, 8, "plain", True, False), _planes(True))
    assert not np.array_equal(a.image()["linear"], b.image()["linear"])
    st = a.render(2)
    assert st["kernel"] == PERLANE and st["tiles"] == 15 and st["samples"] == nx * ny * 2 and st["kernel_ms"] > 0
    c = _session(sc, cam, nx, ny, "nee", False, True)
    assert c.render(2)["kernel"] == sc.render_nee(cam, nx, ny, 2, seed=SEED, flags=FC, coop=True)["stats"]["kernel"]
    d = _session(sc, cam, nx, ny, "nee", False, False)
    assert d.render_for(0.0, 4) == 4 and d.spp() == (4, 4)  # exactly one step
    host.free_all()  # closes the sessions before their scenes
    with pytest.raises(HostError, match="closed"):
        d.render(1)
