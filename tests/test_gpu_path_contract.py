"""GPU tier of tests/test_path_contract.py: the device's production camera_sample, rejection samplers, medium_sample,
transform chains and — world_closest + shade_hit on an uploaded world — material rules, reached through rtmi_probe_path over the same scripted words, are bit-identical to the fp32 oracle —
the words consumed included — and inside the CPU tier's bounds; and a case's result does not depend on which cases share
its wavefront (the corpus in its natural order and under one fixed permutation: wavefronts then mix other trial counts,
other cameras, other chain lengths and another tail).  No kernel here can loop without end: a script that runs out feeds
the samplers the origin, which they accept, and every test asserts that none did."""
import numpy as np
import pytest

import test_path_contract as tc
from raytracing_rust_amd import abi

pytestmark = pytest.mark.gpu


def _run(op, inp, words, **kw):
    """the probe on the cases as they are and under one fixed permutation; the per-case results must be identical"""
    rc, out = tc.probe(op, inp, words, **kw)
    assert rc == 0, abi.load_rtmi().rtmi_last_error()
    perm = np.random.default_rng(123).permutation(len(inp))
    rc, shuffled = tc.probe(op, np.ascontiguousarray(inp[perm]), np.ascontiguousarray(words[perm]), **kw)
    assert rc == 0, abi.load_rtmi().rtmi_last_error()
    back = np.empty_like(shuffled)
    back[perm] = shuffled
    assert np.array_equal(out.view(np.uint32), back.view(np.uint32)), "%d cases depend on their neighbours" % int(
        (out.view(np.uint32) != back.view(np.uint32)).any(axis=1).sum())
    assert not out[:, -1].view(np.uint32).any(), "a script ran out"
    return out, out[:, -2].view(np.uint32)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("dim", [3, 2], ids=["sphere", "disk"])
def test_device_samplers_bit_identical_and_within_bounds(orc32, dim):
    words, cls = tc.sampler_corpus(dim)
    out, used = _run(abi.PROBE_PATH_SPHERE if dim == 3 else abi.PROBE_PATH_DISK, np.zeros((len(words), 1), np.float32), words)
    for i, (p, n, _) in enumerate(tc.orc_sampler(orc32, dim)):
        assert _same(out[i, 0:3], p) and used[i] == n, (i, cls[i], out[i, 0:3], p, used[i], n)
    st, bad = tc.check_sampler([(out[i, 0:3], int(used[i]), False) for i in range(len(words))], dim, "device")
    assert not bad, bad[:10]
    tc.assert_sampler_composition(st, dim)


def test_device_camera_bit_identical_and_within_bounds(orc32, host):
    specs, cams, states, cases, words, cls = tc.camera_corpus(host)
    out, used = _run(abi.PROBE_PATH_CAMERA, cases.view(np.float32), words, cams=states)
    for i, (ray, n, _) in enumerate(tc.orc_camera(orc32, host)):
        assert _same(out[i, 0:7], ray) and used[i] == n, (i, cls[i], cases[i], out[i, 0:7], ray, used[i], n)
    orc32.free_all()
    st, bad = tc.check_camera([(out[i, 0:7], int(used[i]), False) for i in range(len(cases))], host, "device")
    assert not bad, bad[:10]


def test_device_medium_sample_bit_identical_and_within_bounds(orc32):
    rows, dens, words, cls = tc.medium_corpus()
    out, used = _run(abi.PROBE_PATH_MEDIUM_SAMPLE, rows, words)
    for i, (taken, t, n, _) in enumerate(tc.orc_medium(orc32)):
        assert bool(out[i, 0]) == taken and _same(out[i, 1], t) and used[i] == n, (i, cls[i], rows[i], out[i, 0:2], taken, t)
    st, bad = tc.check_medium([(bool(out[i, 0]), float(out[i, 1]), int(used[i]), False) for i in range(len(rows))], "device")
    assert not bad, bad[:10]
    tc.assert_medium_composition(st)


@pytest.mark.parametrize("kind,stream_id", [(0, 0), (1, 0), (2, 3)], ids=["RngRing", "RngReg", "RngNee"])
def test_word_sources_deliver_the_stream_in_order_under_divergence(kind, stream_id):
    """64 lanes of a full wavefront and the 36 of a partial one, 200 steps each: every word a lane is handed equals
    philox.Stream's at that position of its stream, whatever its neighbours draw, skip or restart in the same step"""
    import path_corpus as pc

    lib = abi.load_rtmi()
    seed = 0x0123456789ABCDEF
    for name, script in sorted(pc.stream_scripts(100).items()):
        script = np.ascontiguousarray(script)
        out = np.zeros(script.shape + (3,), np.uint32)
        assert lib.rtmi_probe_stream(kind, seed, script.ctypes.data, script.shape[1], out.ctypes.data, len(script)) == 0, lib.rtmi_last_error()
        want = pc.stream_expected(script, seed, stream_id)
        wrong = np.argwhere((out != want).any(axis=2))
        assert not len(wrong), (name, len(wrong), wrong[:5].tolist(), out[tuple(wrong[0])], want[tuple(wrong[0])])
        draws = int((script > 0).sum() - (script == 4).sum())
        print("%s kind %d: %d draws, %d re-inits, %d idle steps, all words in order" % (name, kind, draws, int((script == 4).sum()), int((script == 0).sum())))
        if name == "render":  # within every step the first wavefront mixes all five kinds of lane
            assert all(len(set(script[:64, s])) >= 3 for s in range(8, script.shape[1])) and set(script[:64].ravel()) == {0, 1, 2, 3, 4}
        else:  # lane 5 is 7 words ahead of its neighbours from step 3 on
            assert script[5, :3].tolist() == [3, 3, 1] and not script[[4, 6], :3].any() and (script[4, 3:] == script[5, 3:]).all()


def test_device_chain_round_trip_bit_identical_and_within_bounds(orc32, host):
    specs, xforms, first, count, rows, idx = tc.chain_corpus(host)
    inp = np.zeros((len(rows), abi.PROBE_PATH_IN), np.float32)
    inp[:, 0:7] = rows[:, 0:7]
    inp[:, 7] = np.array([first[s] for s in idx], np.int32).view(np.float32)
    inp[:, 8] = np.array([count[s] for s in idx], np.int32).view(np.float32)
    inp[:, 9:12] = rows[:, 7:10]
    out, used = _run(abi.PROBE_PATH_XFORM_ROUNDTRIP, inp, np.zeros((len(rows), abi.PROBE_PATH_WORDS), np.uint32), xforms=xforms)
    assert not used.any()
    for i, (p, n) in enumerate(tc.orc_chain(orc32, host)):
        assert _same(out[i, 0:3], p) and _same(out[i, 3:6], n), (i, specs[idx[i]][0], out[i, 0:6], p, n)
    st, bad = tc.check_chain([(out[i, 0:3], out[i, 3:6]) for i in range(len(rows))], host, "device")
    assert not bad, bad[:10]


def _same_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("face_forward", [0, 1])
def test_device_bounce_bit_identical_and_within_bounds(orc32, host, face_forward):
    """world_closest + shade_hit over the uploaded hand-built world: the hit, the scatter decision, the scattered ray, T, L
    and the words consumed equal the fp32 oracle's bit for bit (NaN for NaN in the out-of-range direction-magnitude cases:
    this is what pins the device there), the material rules hold their exact bounds on the device's own output, and
    (closest, item, primitive) and the scattered origin equal rtmi_trace's record of the same rays."""
    import ctypes as C

    import path_corpus as pc
    from oracle.oracle import ARITH_DEVICE, FACE_FORWARD

    lib = abi.load_rtmi()
    rows, words, cls, obj, scale = tc.bounce_corpus()
    low = host.lower(pc.bounce_world(host))
    desc = low.desc()
    scene = C.c_void_p()
    assert lib.rtmi_scene_create(C.byref(desc), 0, C.byref(scene)) == 0, lib.rtmi_last_error()
    try:
        inp = np.zeros((len(rows), abi.PROBE_PATH_IN), np.float32)
        inp[:, 0:9] = rows[:, 0:9]
        inp[:, 9] = rows[:, 9].astype(np.uint32).view(np.float32)
        inp[:, 10] = np.uint32(pc.BOUNCE_MAX_DEPTH).view(np.float32)
        inp[:, 11] = np.uint32(abi.RTMI_FLAG_FACE_FORWARD if face_forward else 0).view(np.float32)
        out, used = _run(abi.PROBE_PATH_BOUNCE, inp, words, scene=scene)
        # refused before any device work: a flag that is no extension of shade_hit, and cases that differ in a launch's values
        for col, value, rows_hit in ((11, abi.RTMI_FLAG_SKY, slice(None)), (11, abi.RTMI_FLAG_UV_BOOK, slice(5, 6)), (10, 7, slice(63, 64))):
            wrong = inp[:64].copy()
            wrong[rows_hit, col] = np.uint32(value).view(np.float32)
            assert tc.probe(abi.PROBE_PATH_BOUNCE, wrong, words[:64], scene=scene)[0] == 1, (col, value)
    finally:
        lib.rtmi_scene_destroy(scene)
    ref = tc.orc_bounce(orc32, ARITH_DEVICE | (FACE_FORWARD if face_forward else 0))
    dev = []
    for i, b in enumerate(ref):
        o = out[i]
        hit = bool(np.isfinite(o[0])) or bool(np.isnan(o[0]))
        assert hit == (b is not None), (i, cls[i], o[0:5], b)
        if b is None:
            assert used[i] == 0 or pc.BOUNCE_OBJECTS[obj[i]][0] == "fog"
            dev.append(None)
            continue
        assert _same_or_nan(o[0], b["t"]) and bool(o[4]) == b["scattered"] and used[i] == b["consumed"], (i, cls[i], scale[i], o, b)
        assert _same_or_nan(o[11:14], b["T"]) and _same_or_nan(o[14:17], b["L"]), (i, cls[i], o, b)
        if b["scattered"]:
            assert _same_or_nan(o[5:8], b["o"]) and _same_or_nan(o[8:11], b["d"]), (i, cls[i], scale[i], o, b)
        dev.append(dict(b, t=float(o[0]), scattered=bool(o[4]), o=o[5:8].astype(np.float64), d=o[8:11].astype(np.float64),
                        T=o[11:14].astype(np.float64), L=o[14:17].astype(np.float64), consumed=int(used[i]), exhausted=False))
    st, bad = tc.check_bounce(dev, face_forward, "device")
    assert not bad, bad[:10]
    tc.assert_bounce_composition(st, face_forward)
    # rtmi_trace of the same rays, the scaled class and the in-plane (t = NaN) rays included; its medium draws are
    # Philox's, not the script's, so the rays aimed at the fog are left out
    keep = np.array([pc.BOUNCE_OBJECTS[obj[i]][0] != "fog" for i in range(len(rows))])
    up = host.lower(pc.bounce_world(host)).upload(0)
    tr = up.trace(rows[keep, 0:3], rows[keep, 3:6], t_min=rows[keep, 7], t_max=rows[keep, 8], flags=0)
    k = np.flatnonzero(keep)
    assert _same_or_nan(out[k, 0], tr["t"]) and np.array_equal(out[k, 1].view(np.int32), tr["item"]) and np.array_equal(out[k, 2].view(np.int32), tr["prim"])
    went_on = out[k, 4] != 0
    assert went_on.sum() >= 300 and _same_or_nan(out[k][went_on, 5:8], tr["p"][went_on])
